"""Host side of the exact DECIMAL SUM / AVG aggregates: the general 40-B
DecimalStructure codecs of chunk.py against hand-laid-out byte patterns, the
spec bit layout, the partial->final mapping and the wire round trip of wide
records. No GPU."""
import ctypes as C
import random
import struct

import numpy as np
import pytest

from galaxysql_amd import abi
from galaxysql_amd.chunk import (Block, Chunk, DECIMAL, I64, dec40_decode,
                                 dec40_decode_wide, dec40_encode,
                                 dec40_encode_wide)
from galaxysql_amd.exchange import final_agg_specs
from galaxysql_amd.serde import deserialize_chunk, serialize_chunk

from . import decsum_ref as ref


def test_golden_vectors_both_ways():
    vecs = ref.load_golden()["vectors"]
    # 1, 2, 3 and 5 integer words, negatives, zero, scales 0 / 2 / 9
    assert {len(v["int_words"]) for v in vecs} >= {1, 2, 3, 5}
    assert {v["scale"] for v in vecs} >= {0, 2, 9}
    assert any(v["neg"] for v in vecs) and any(v["scaled"] == "0" for v in vecs)
    for v in vecs:
        want = bytes.fromhex(v["hex"])
        scaled, scale = int(v["scaled"]), v["scale"]
        assert len(want) == 40
        assert dec40_encode_wide(scaled, scale) == want, v["note"]
        assert dec40_decode_wide(want) == (scaled, scale), v["note"]
        assert ref.decode_general(want) == (scaled, scale), v["note"]


def _record(words, integers, fractions, neg):
    p = bytearray(40)
    struct.pack_into(f"<{len(words)}i", p, 0, *words)
    p[36], p[37], p[38], p[39] = integers, fractions, fractions, neg
    return bytes(p)


def test_decode_general_layout():
    """Layouts the encoder never writes: digit counts that are no multiple
    of 9, no integer word at all, two fraction words."""
    cases = [
        (_record([123, 450000000], 3, 2, 0), (12345, 2)),
        (_record([500000000], 0, 1, 1), (-5, 1)),              # -0.5
        (_record([7, 123456789, 120000000], 1, 11, 0),
         (7 * 10 ** 11 + 12345678912, 11)),                     # 2 frac words
        (_record([1, 0, 5], 10, 9, 0), ((10 ** 9) * 10 ** 9 + 5, 9)),
    ]
    for p, want in cases:
        assert dec40_decode_wide(p) == want
        assert ref.decode_general(p) == want


def test_wide_matches_simple_encoder():
    rng = random.Random(7)
    for _ in range(4000):
        scale = rng.randrange(0, 10)
        v = rng.randrange(-10 ** 18 + 1, 10 ** 18)
        if rng.random() < 0.2:
            v = rng.randrange(-1000, 1000)
        p = dec40_encode_wide(v, scale)
        assert p == dec40_encode(v, scale)
        assert dec40_decode_wide(p) == (v, scale)
        assert ref.decode_general(p) == (v, scale)
        # the simple decoder raises on values that leave scaled-int64 range
        if abs(v) // 10 ** scale < 10 ** (18 - scale):
            assert dec40_decode(p, scale) == v


def test_simple_codecs_keep_their_limit():
    with pytest.raises(ValueError):
        dec40_encode(10 ** 18, 0)
    wide = dec40_encode_wide(10 ** 20, 0)
    with pytest.raises(ValueError):
        dec40_decode(wide, 0)


def test_wide_encoder_limits():
    assert dec40_decode_wide(dec40_encode_wide(2 ** 127 - 1, 0)) == \
        (2 ** 127 - 1, 0)
    with pytest.raises(ValueError):
        dec40_encode_wide(10 ** 72, 0)   # 9 integer words + fraction word
    with pytest.raises(ValueError):
        dec40_encode_wide(1, 10)


def test_spec_bit_layout():
    assert (abi.SUM_DEC, abi.AVG_DEC) == (28, 29)
    for s in range(10):
        f = abi.sum_dec(s)
        assert f == 28 | (s << 16)
        assert abi.base_func(f) == abi.SUM_DEC and abi.func_scale(f) == s
    assert abi.avg_dec(4) == 29 | (4 << 16)
    assert abi.sum_dec(0) == abi.SUM_DEC
    # every existing func has zero upper bits
    for f in range(28):
        assert abi.base_func(f) == f and abi.func_scale(f) == 0
    # the spec struct carries it unchanged
    sp = abi.GxAggSpec(abi.sum_dec(9), 3)
    assert sp.func == 0x9001C and sp.input_col == 3


def test_final_agg_specs_mapping():
    finals, types = final_agg_specs(
        2, [(abi.COUNT_ROW, -1), (abi.sum_dec(2), 5), (abi.sum_dec(0), 6)])
    assert finals == [(abi.SUM_I64, 2), (abi.sum_dec(2), 3),
                      (abi.sum_dec(0), 4)]
    assert types == [I64, DECIMAL, DECIMAL]
    with pytest.raises(ValueError, match="partial SUM_DEC\\+COUNT"):
        final_agg_specs(1, [(abi.avg_dec(2), 1)])
    with pytest.raises(ValueError, match="partial SUM\\+COUNT"):
        final_agg_specs(1, [(abi.AVG_F64, 1)])


def _wide_chunk():
    rng = random.Random(11)
    vals = []
    for i in range(300):
        if i % 7 == 0:
            vals.append(None)
        else:
            digits = rng.choice([3, 17, 19, 28, 38])
            v = rng.randrange(10 ** (digits - 1), 10 ** digits)
            vals.append(-v if rng.random() < 0.5 else v)
    return vals, Chunk([ref.dec_block(vals, scale=2),
                        Block(I64, values=np.arange(300, dtype=np.int64))])


def test_serde_python_roundtrip_wide():
    vals, c = _wide_chunk()
    buf = serialize_chunk(c)
    back, _pos = deserialize_chunk(buf, [DECIMAL, I64])
    got = [None if v is None else ref.decode_cell(v)
           for v in (back.blocks[0].get(i) for i in range(300))]
    assert got == [None if v is None else (v, 2) for v in vals]


def test_serde_native_roundtrip_wide():
    """gxop_chunk_serialize / deserialize of the oracle build: wide records
    are opaque 40-B payload, byte-identical to the Python writer."""
    abi.load_oracle()   # built?
    # a private handle: the argtypes set here must not leak into the cached
    # library object other test modules share
    lib = abi.GxLib(abi.ORACLE_PATH)
    L = lib.lib
    L.gxop_chunk_serialize.restype = C.c_int
    L.gxop_chunk_serialize.argtypes = [C.c_void_p,
                                       C.POINTER(C.POINTER(C.c_uint8)),
                                       C.POINTER(C.c_int64)]
    L.gxop_chunk_deserialize.restype = C.c_int
    L.gxop_chunk_deserialize.argtypes = [C.POINTER(C.c_uint8), C.c_int64,
                                         C.POINTER(C.c_int32), C.c_int32,
                                         C.POINTER(C.c_void_p),
                                         C.POINTER(C.c_int64)]
    vals, c = _wide_chunk()
    ka = []
    gc = lib.to_gx_chunk(c, ka)
    out = C.POINTER(C.c_uint8)()
    n = C.c_int64()
    assert L.gxop_chunk_serialize(C.byref(gc), C.byref(out), C.byref(n)) == 0
    buf = bytes(C.cast(out, C.POINTER(C.c_uint8 * n.value)).contents)
    L.gxop_buf_free(out)
    assert buf == serialize_chunk(c)
    arr = (C.c_uint8 * len(buf)).from_buffer_copy(buf)
    types = (C.c_int32 * 2)(DECIMAL, I64)
    outc = C.c_void_p()
    consumed = C.c_int64()
    assert L.gxop_chunk_deserialize(C.cast(arr, C.POINTER(C.c_uint8)),
                                    len(buf), types, 2, C.byref(outc),
                                    C.byref(consumed)) == 0, lib.error()
    assert consumed.value == len(buf)
    g = C.cast(outc, C.POINTER(abi.GxChunk)).contents
    assert g.n_rows == 300
    recs = np.ctypeslib.as_array(
        C.cast(g.blocks[0].values, C.POINTER(C.c_uint8)), shape=(300, 40))
    for i, v in enumerate(vals):
        if v is not None:
            assert bytes(recs[i]) == bytes(c.blocks[0].values[i])
            assert ref.decode_cell(recs[i]) == (v, 2)
    L.gxop_chunk_free(outc)


def test_ref_avg_half_up():
    # ties round away from zero on the magnitude
    assert ref.avg4(1, 2 * 10 ** 4, 0) == 1          # 0.00005 -> 0.0001
    assert ref.avg4(-1, 2 * 10 ** 4, 0) == -1
    assert ref.avg4(1, 3, 0) == 3333
    assert ref.avg4(2, 3, 0) == 6667
    assert ref.avg4(-2, 3, 0) == -6667
    assert ref.avg4(12345, 1, 2) == 1234500
    assert ref.avg4(5, 2, 4) == 3                     # 0.00025 -> 0.0003


def test_dec128_header_on_host(tmp_path):
    """The 128-bit helpers the kernels use (csrc/gx_dec128.h: record decode
    with its fences, record encode, long division, AVG rounding), compiled
    for the host and compared with Python integers."""
    import os
    import subprocess
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "dec128_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I",
                    os.path.join(repo, "galaxysql_amd", "csrc"),
                    os.path.join(repo, "tools", "dec128_check.cpp"),
                    "-o", exe], check=True, capture_output=True)
    rng = random.Random(5)
    M64 = 2 ** 64 - 1
    lines, want = [], []

    def split(v):
        return v >> 64, v & M64

    for _ in range(1500):
        # decode: in-range values at the aggregate's scale or a smaller one
        s = rng.randrange(0, 10)
        f = rng.randrange(0, s + 1)
        digits = rng.randrange(1, 30 - (s - f))
        v = rng.randrange(0, 10 ** digits)
        if v * 10 ** (s - f) >= 10 ** 29:
            continue
        neg = rng.random() < 0.5 and v != 0
        rec = dec40_encode_wide(-v if neg else v, f)
        lines.append(f"D {rec.hex()} {s}")
        hi, lo = split(v * 10 ** (s - f))
        want.append(f"0 {int(neg)} {hi} {lo}")
    # fences: fractions > scale, 10 words, magnitude
    lines.append(f"D {dec40_encode_wide(12345, 5).hex()} 2")
    want.append("1 0 0 0")
    lines.append(f"D {_record([1] * 9, 82, 0, 0).hex()} 0")
    want.append("2 0 0 0")
    lines.append(f"D {_record([1] * 8, 64, 11, 0).hex()} 9")
    want.append("2 0 0 0")
    lines.append(f"D {dec40_encode_wide(10 ** 29, 0).hex()} 0")
    want.append("4 0 0 0")
    lines.append(f"D {dec40_encode_wide(-(10 ** 27), 0).hex()} 2")
    want.append("4 1 0 0")
    lines.append(f"D {dec40_encode_wide(10 ** 29 - 1, 0).hex()} 0")
    want.append("0 0 %d %d" % split(10 ** 29 - 1))
    lines.append(f"D {dec40_encode_wide(10 ** 71, 0).hex()} 0")   # 8 words
    want.append("4 0 0 0")
    for _ in range(1500):
        # encode any magnitude below 2^128
        s = rng.randrange(0, 10)
        v = rng.randrange(0, 2 ** rng.randrange(1, 129))
        neg = rng.random() < 0.5
        lines.append("E %d %d %d %d" % (*split(v), int(neg), s))
        want.append(dec40_encode_wide(-v if neg else v, s).hex())
    for _ in range(1500):
        v = rng.randrange(0, 2 ** rng.randrange(1, 129))
        d = rng.randrange(1, 2 ** rng.choice([1, 20, 32, 33, 50, 64]))
        lines.append("Q %d %d %d" % (*split(v), d))
        want.append("%d %d %d" % (*split(v // d), v % d))
    for _ in range(1500):
        s = rng.randrange(0, 5)
        c = rng.randrange(1, 2 ** rng.choice([1, 8, 31, 32, 33, 63]))
        v = rng.randrange(0, 2 ** rng.randrange(1, 113))
        if rng.random() < 0.3:   # exact .5 ties
            k = rng.randrange(1, 10 ** 6)
            c = 2 * 10 ** (4 - s) * k
            v = k * (2 * rng.randrange(0, 10 ** 9) + 1)
        lines.append("A %d %d %d %d" % (*split(v), c, s))
        want.append("%d %d" % split(ref.avg4(v, c, s)))
    r = subprocess.run([exe], input="\n".join(lines) + "\n",
                       capture_output=True, text=True, check=True)
    got = r.stdout.split("\n")[:-1]
    assert len(got) == len(want)
    for line, g, w in zip(lines, got, want):
        assert g == w, (line, g, w)
