"""csrc/gx_agg_layout.h on the host: the aggregate state record's layout rule,
AggLayout::select, the result types and agg_decode, through
tools/agg_layout_check.cpp, against the rule written out here from the
gx_agg_func comments of include/gxop.h (which funcs start NULL, what the
others start from, SUM_DEC / AVG_DEC's 128-bit sum, AVG's {sum, count})."""
import os
import struct
import subprocess

import pytest

(COUNT_ROW, COUNT_COL, SUM_I64, SUM_F64, MIN_I64, MAX_I64, MIN_F64, MAX_F64,
 AVG_F64, BIT_AND, BIT_OR, BIT_XOR) = range(12)
SUM_I64N, SUM_DEC, AVG_DEC = 22, 28, 29
GX_I64, GX_F64, GX_DECIMAL = 0, 2, 4
GX_MAX_COLS = 16

ALL13 = [COUNT_ROW, COUNT_COL, SUM_I64, SUM_I64N, SUM_F64, AVG_F64, MIN_I64,
         MAX_I64, MIN_F64, MAX_F64, BIT_AND, BIT_OR, BIT_XOR]
Q1 = [SUM_DEC] * 4 + [AVG_DEC] * 3 + [COUNT_ROW]

NEVER_NULL = {COUNT_ROW, COUNT_COL, SUM_I64, BIT_AND, BIT_OR, BIT_XOR}
DEC = {SUM_DEC, AVG_DEC}
F64 = {SUM_F64, MIN_F64, MAX_F64, AVG_F64}


def f64_bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def identity(f):
    return {MIN_I64: 2 ** 63 - 1, MAX_I64: 2 ** 63,
            MIN_F64: f64_bits(float("inf")), MAX_F64: f64_bits(-float("inf")),
            BIT_AND: 2 ** 64 - 1}.get(f, 0)


def model(funcs):
    """(stride, val_off, seen_off, tmpl)"""
    val, seen, tmpl = [], [], []
    for f in funcs:
        val.append(len(tmpl))
        tmpl.append(identity(f))
        if f in DEC:
            tmpl.append(0)          # hi word of the 128-bit sum
        if f in NEVER_NULL:
            seen.append(-1)
        else:
            seen.append(len(tmpl))  # seen flag / AVG's count
            tmpl.append(0)
    if not tmpl:
        tmpl = [0]
    return len(tmpl), val, seen, tmpl


def result_type(f):
    return GX_DECIMAL if f in DEC else GX_F64 if f in F64 else GX_I64


def ints(v):
    return " |" + "".join(f" {x}" for x in v)


def want_L(funcs):
    stride, val, seen, tmpl = model(funcs)
    return (f"{stride}{ints(val)}{ints(seen)} |" +
            "".join(f" {w:x}" for w in tmpl) +
            f" | {int(not any(tmpl))}{ints(result_type(f) for f in funcs)}")


def want_S(funcs, idx):
    stride, val, seen, _ = model(funcs)
    return (f"{len(idx)} {stride}{ints(funcs[i] for i in idx)}"
            f"{ints(val[i] for i in idx)}{ints(seen[i] for i in idx)}")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path_factory.mktemp("agg_layout") / "agg_layout_check")
    subprocess.run(["g++", "-O1", "-std=c++17",
                    "-I", os.path.join(repo, "galaxysql_amd", "csrc"),
                    "-I", os.path.join(repo, "include"),
                    os.path.join(repo, "tools", "agg_layout_check.cpp"),
                    "-o", out], check=True, capture_output=True)
    return out


def cases():
    """(input line, expected output line)"""
    out = []
    lists = [[f] for f in ALL13 + [SUM_DEC, AVG_DEC]]
    lists += [ALL13, Q1, [],
              # DEC funcs mixed in; the second list's only non-zero identity
              # lies behind a DEC record, past the first aggregates' slots
              [COUNT_ROW, SUM_DEC, MIN_F64, AVG_DEC, SUM_I64N, BIT_AND],
              [SUM_DEC, AVG_DEC, COUNT_COL, MAX_I64],
              [SUM_DEC, AVG_DEC, SUM_I64],
              [AVG_DEC] * GX_MAX_COLS]
    for funcs in lists:
        line = " ".join(map(str, funcs))
        out.append((f"L {line}", want_L(funcs)))
    for funcs, idx in [(ALL13, [0, 2, 4]), (ALL13, [12, 5, 3]),
                       (ALL13, list(range(13))), (ALL13, []),
                       (Q1, [7, 4, 0]),
                       ([COUNT_ROW, SUM_DEC, MIN_F64, AVG_DEC], [3, 1])]:
        out.append((f"S {' '.join(map(str, funcs))} | "
                    f"{' '.join(map(str, idx))}", want_S(funcs, idx)))
    # decode: a SUM whose seen slot holds 5 (the transposed accumulate adds
    # to it) is non-null with its value unchanged
    for f, v in ((SUM_I64N, 0xFFFFFFFFFFFFFF85), (SUM_F64, f64_bits(-12.5))):
        out.append((f"V {f} {v:x} 5", f"{v:x} 0"))
    # AVG = sum / count
    for s, n in ((10.0, 3), (-7.0, 3), (1e300, 1), (0.0, 7)):
        out.append((f"V {AVG_F64} {f64_bits(s):x} {n:x}",
                    f"{f64_bits(s / float(n)):x} 0"))
    # a NULL of every null-tracking func decodes to zero bits whatever the
    # value slot holds; the others are never NULL and ignore the seen word
    for f in ALL13:
        v = identity(f) or 0x1234
        if f in NEVER_NULL:
            out.append((f"V {f} {v:x} 0", f"{v:x} 0"))
        else:
            out.append((f"V {f} {v:x} 0", "0 1"))
            if f != AVG_F64:
                out.append((f"V {f} {v:x} 1", f"{v:x} 0"))
    return out


def test_model_matches_documented_records():
    assert model(Q1)[0] == 22            # Q1's 22-u64 record
    assert model([COUNT_ROW, SUM_I64])[0] == 2
    stride = model([AVG_DEC] * GX_MAX_COLS)[0]
    assert stride == 3 * GX_MAX_COLS     # the widest record fits tmpl
    # tmpl_zero is decided over the whole stride
    assert want_L([SUM_DEC, AVG_DEC, COUNT_COL, MAX_I64]).split(" | ")[-2] \
        == "0"
    assert want_L([SUM_DEC, AVG_DEC, SUM_I64]).split(" | ")[-2] == "1"


def test_header_on_host(exe):
    cs = cases()
    p = subprocess.run([exe], input="".join(c[0] + "\n" for c in cs),
                       capture_output=True, text=True, check=True)
    got = p.stdout.splitlines()
    assert len(got) == len(cs)
    for (line, want), g in zip(cs, got):
        assert g == want, (line, g, want)
    # the widest record: stride within the template's 3 * GX_MAX_COLS words
    widest = [g for (line, _), g in zip(cs, got)
              if line == "L " + " ".join([str(AVG_DEC)] * GX_MAX_COLS)]
    assert int(widest[0].split()[0]) <= 3 * GX_MAX_COLS
