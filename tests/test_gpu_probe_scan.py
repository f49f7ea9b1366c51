"""Fused scan+probe (gxop_join_probe_scan) parity.

Every case compares three row multisets, sorted by all columns:
  (a) the fused call on the HIP library, raw chunk device-resident (the
      only residency the fast path takes);
  (b) gxop_scan_consume then gxop_join_probe on the same HIP library;
  (c) scan then probe on the CPU oracle.
Integers and doubles must match exactly (per-row expressions, nothing is
reordered), and n_scan_kept must equal the composed scan's row count.
"""
import ctypes as C

import numpy as np
import pytest

from galaxysql_amd import abi
from galaxysql_amd.abi import GxResult
from galaxysql_amd.chunk import (Block, Chunk, I64, I32, F64, SLICE, DECIMAL,
                                 multiset)
from galaxysql_amd.operators import (ParallelHashJoinExec, ScanExec,
                                     EquiJoinKey, JoinCond)

pytestmark = pytest.mark.gpu

# raw probe-side table: key, date (predicate column), price f64, disc f64,
# price cents, disc hundredths
RAW_TYPES = [I64, I32, F64, F64, I64, I64]
PROJS = [(abi.PROJ_COPY, 0, -1), (abi.PROJ_REV_F64, 2, 3),
         (abi.PROJ_REV_SCALED4, 4, 5), (abi.PROJ_COPY, 1, -1)]
OUT_TYPES = [I64, F64, I64, I32]        # what PROJS produce
BUILD_TYPES = [I64, I32]                # key, payload
PRED_CUT = {"none": 1000, "all": -1, "half": 49}   # date > cut, date in [0,100)
BIG_BUILD = 70_000      # >= 65536 rows: the size at which enable_bloom acts


def gen_build(rng, n_keys, dup=1, with_nulls=True):
    keys = np.repeat(np.arange(n_keys, dtype=np.int64) * 3 + 1, dup)
    rng.shuffle(keys)
    pay = rng.integers(0, 1000, len(keys)).astype(np.int32)
    kn = pn = None
    if with_nulls:
        kn = (rng.random(len(keys)) < 0.02).astype(np.uint8)
        pn = (rng.random(len(keys)) < 0.05).astype(np.uint8)
    return [(keys, kn), (pay, pn)]


def gen_raw(rng, n, n_keys, match, null_cols):
    """match: 'none' (keys outside the build's), 'all', or 'tenth'."""
    if match == "none":
        key = rng.integers(0, max(n_keys, 1), n).astype(np.int64) * 3 + 2
    elif match == "all":
        key = rng.integers(0, max(n_keys, 1), n).astype(np.int64) * 3 + 1
    else:
        key = rng.integers(0, 10 * max(n_keys, 1), n).astype(np.int64) * 3 + 1
    date = rng.integers(0, 100, n).astype(np.int32)
    cents = rng.integers(100, 10_000_000, n).astype(np.int64)
    disc = rng.integers(0, 11, n).astype(np.int64)
    vals = [key, date, cents.astype(np.float64) / 100.0,
            disc.astype(np.float64) / 100.0, cents, disc]
    cols = []
    for c, v in enumerate(vals):
        nl = None
        if c in null_cols:
            nl = (rng.random(n) < 0.07).astype(np.uint8)
        cols.append((v, nl))
    return cols


def host_chunk(cols, types):
    return Chunk([c if isinstance(c, Block) else
                  Block(t, values=c[0], nulls=c[1])
                  for c, t in zip(cols, types)])


def dev_chunk(lib, cols, types, ka):
    """GxChunk over device copies of the columns (mem = DEVICE)."""
    import torch

    def up(a):
        t = torch.from_numpy(np.array(a)).cuda()
        ka.append(t)
        return t.data_ptr() if t.numel() else None

    ptrs = []
    for c, ty in zip(cols, types):
        if isinstance(c, Block):      # SLICE
            d = {"type": ty, "n_rows": c.n_rows, "offsets": up(c.offsets),
                 "data": up(c.data), "data_len": int(len(c.data))}
            if c.nulls is not None:
                d["nulls"] = up(c.nulls)
        else:
            d = {"type": ty, "n_rows": len(c[0]), "values": up(c[0])}
            if c[1] is not None:
                d["nulls"] = up(c[1])
        ptrs.append(d)
    return lib.to_gx_chunk(None, ka, device_ptrs=ptrs)


def canon(chunk, n_cols):
    """Row multiset as a lexsorted int64 matrix (null flag, value bits per
    column; NULL slots masked to 0). SLICE columns: python multiset."""
    if chunk is None or chunk.n_rows == 0:
        return np.zeros((0, 2 * n_cols), np.int64)
    if any(b.type == SLICE for b in chunk.blocks):
        return multiset(chunk.rows())
    n = chunk.n_rows
    cols = []
    for b in chunk.blocks:
        nl = (b.nulls.astype(np.int64) if b.nulls is not None
              else np.zeros(n, np.int64))
        if b.type == DECIMAL:
            v = np.ascontiguousarray(b.values).view(np.int64).reshape(n, 5)
            vs = [np.where(nl != 0, 0, v[:, k]) for k in range(5)]
        elif b.type == F64:
            vs = [np.where(nl != 0, 0,
                           np.ascontiguousarray(b.values).view(np.int64))]
        else:
            vs = [np.where(nl != 0, 0, b.values.astype(np.int64))]
        cols.append(nl)
        cols.extend(vs)
    m = np.stack(cols, axis=1)
    return m[np.lexsort(m.T[::-1])]


def same(a, b):
    if isinstance(a, np.ndarray) and isinstance(b, np.ndarray):
        return a.shape[0] == b.shape[0] and (a.shape[0] == 0 or
                                             np.array_equal(a, b))
    return a == b


def run_case(raw_cols, build_cols, preds, *, join_type=abi.INNER,
             keys=None, raw_types=RAW_TYPES, projs=PROJS,
             out_types=OUT_TYPES, build_types=BUILD_TYPES, out_proj=None,
             enable_bloom=False, conds=None, anti_null_col=-1,
             null_free=False):
    hip = abi.load_hip()
    oracle = abi.load_oracle()
    assert hip.has_probe_scan and not oracle.has_probe_scan
    keys = keys or [EquiJoinKey(0, 0, I64)]
    semi = join_type in (abi.SEMI, abi.ANTI)
    n_full = len(out_types) + (0 if semi else len(build_types))
    n_out = len(out_proj) if out_proj else n_full
    build = host_chunk(build_cols, build_types)

    def make(lib, device):
        j = ParallelHashJoinExec(lib, join_type, keys, out_types, build_types,
                                 device=device, out_proj=out_proj,
                                 enable_bloom=enable_bloom, conds=conds,
                                 anti_null_col=anti_null_col)
        s = ScanExec(lib, preds, projs, raw_types, device=device)
        j.consume_chunk(build)
        j.build_consume()
        return j, s

    # (c) oracle, composed
    j, s = make(oracle, -1)
    try:
        t = s.consume_chunk(host_chunk(raw_cols, raw_types))
        kept_c = t.n_rows if t is not None else 0
        ref = j.probe_chunk(t) if kept_c else None
    finally:
        j.close()
        s.close()
    ref = canon(ref, n_out)

    j, s = make(hip, 0)
    try:
        ka = []
        gc = dev_chunk(hip, raw_cols, raw_types, ka)
        # (a) fused
        out, kept_a = j.probe_scan(s, C.byref(gc))
        chunk_a = hip.result_to_chunk(out) if out else None
        got_a = canon(chunk_a, n_out)
        # (b) composed on the same library and the same built join
        t = s.consume_raw(C.byref(gc))
        kept_b = t.contents.chunk.n_rows
        out = C.POINTER(GxResult)()
        hip.check(hip.lib.gxop_join_probe(j._op, C.byref(t.contents.chunk),
                                          C.byref(out)), "join_probe")
        chunk_b = hip.result_to_chunk(out) if out else None
        got_b = canon(chunk_b, n_out)
        hip.lib.gxop_result_release(t)
    finally:
        j.close()
        s.close()
    n_rows = len(got_b) if isinstance(got_b, np.ndarray) \
        else sum(got_b.values())
    print(f"kept fused/composed/oracle = {kept_a}/{kept_b}/{kept_c}, "
          f"rows = {n_rows}")
    assert kept_a == kept_b == kept_c
    assert same(got_b, ref), "composed HIP != oracle"
    assert same(got_a, got_b), "fused != composed HIP"
    assert same(got_a, ref), "fused != oracle"
    if null_free and n_rows:
        # null-free inputs: the result blocks carry no nulls array at all
        for ch in (chunk_a, chunk_b):
            assert all(b.nulls is None for b in ch.blocks)
    return n_rows


ALL_NULLS = (0, 1, 2, 3, 4, 5)


@pytest.fixture(scope="module")
def small_build():
    return gen_build(np.random.default_rng(7001), 300)


@pytest.fixture(scope="module")
def big_build():
    return gen_build(np.random.default_rng(7002), BIG_BUILD)


@pytest.mark.parametrize("nulls", ["nulls", "nullfree"])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 100_003])
def test_row_counts(n, nulls, small_build):
    """Wave / block edges, and ~100k rows: several grid-stride iterations
    and mid-kernel flushes of the 512-pair emit stage."""
    rng = np.random.default_rng(100 + n)
    build = small_build if nulls == "nulls" else \
        gen_build(np.random.default_rng(7003), 300, with_nulls=False)
    raw = gen_raw(rng, n, 300, "all",
                  ALL_NULLS if nulls == "nulls" else ())
    rows = run_case(raw, build, [(1, abi.GT, PRED_CUT["half"])],
                    null_free=(nulls == "nullfree"))
    if n >= 63:
        assert rows > 0


@pytest.mark.parametrize("match", ["none", "all", "tenth"])
@pytest.mark.parametrize("pred", ["none", "all", "half"])
def test_selectivity(pred, match, big_build):
    """Predicate passes none / all / ~half; build keys match none (with the
    bloom filter on, it rejects everything), all, or ~10 %."""
    rng = np.random.default_rng(200 + 3 * list(PRED_CUT).index(pred) +
                                ["none", "all", "tenth"].index(match))
    raw = gen_raw(rng, 30_011, BIG_BUILD, match, (0, 1))
    rows = run_case(raw, big_build, [(1, abi.GT, PRED_CUT[pred])],
                    enable_bloom=True)
    assert (rows > 0) == (pred != "none" and match != "none")


@pytest.mark.parametrize("null_col", [0, 1, 2, 3, 4, 5])
def test_null_in_one_column(null_col, small_build):
    """NULLs in the key column, the predicate column, and each operand of
    REV_F64 / REV_SCALED4, one at a time."""
    rng = np.random.default_rng(300 + null_col)
    raw = gen_raw(rng, 4099, 300, "tenth", (null_col,))
    assert run_case(raw, small_build, [(1, abi.GT, PRED_CUT["half"])]) > 0


@pytest.mark.parametrize("bloom", [0, 1])
@pytest.mark.parametrize("join_type,out_proj", [
    (abi.INNER, None), (abi.INNER, [0, 2, 5]), (abi.INNER, [4, 5]),
    (abi.SEMI, None), (abi.SEMI, [1, 3])])
def test_join_shapes(join_type, out_proj, bloom, big_build):
    """INNER and SEMI; bloom off and on; all output columns, a subset, and
    only build-side columns."""
    rng = np.random.default_rng(400 + bloom)
    raw = gen_raw(rng, 20_001, BIG_BUILD, "tenth", ALL_NULLS)
    rows = run_case(raw, big_build, [(1, abi.GT, PRED_CUT["half"])],
                    join_type=join_type, out_proj=out_proj,
                    enable_bloom=bool(bloom))
    assert rows > 0


def test_bucket_overflow():
    """Build keys duplicated 6x: buckets run past their 4 inline slots."""
    rng = np.random.default_rng(500)
    build = gen_build(rng, 500, dup=6)
    raw = gen_raw(rng, 5003, 500, "all", ALL_NULLS)
    assert run_case(raw, build, [(1, abi.GT, PRED_CUT["half"])]) > 5003


def test_pair_list_retry():
    """40 000 raw rows all pass and each matches 4 build rows: 160 000
    pairs exceed the first-attempt capacity max(2n, 65536) and force the
    exact-size retry."""
    rng = np.random.default_rng(501)
    build = gen_build(rng, 1000, dup=4, with_nulls=False)
    raw = gen_raw(rng, 40_000, 1000, "all", ())
    assert run_case(raw, build, [(1, abi.GT, PRED_CUT["all"])]) == 160_000


def test_other_projections(small_build):
    """Q9_AMOUNT4 and SCALED_TO_DEC evaluated late, DECIMAL output."""
    rng = np.random.default_rng(502)
    raw = gen_raw(rng, 3001, 300, "all", (0, 4, 5))
    projs = [(abi.PROJ_COPY, 0, -1), (abi.PROJ_Q9_AMOUNT4, 4, 5, 5, 4),
             (abi.PROJ_SCALED_TO_DEC, 4, -1, 2)]
    assert run_case(raw, small_build, [(1, abi.GT, PRED_CUT["half"])],
                    projs=projs, out_types=[I64, I64, DECIMAL]) > 0


# ---- shapes outside the fast path: the composed sequence in the library ----

def test_fallback_anti_not_in():
    rng = np.random.default_rng(600)
    build = [gen_build(rng, 300, with_nulls=False)[0]]
    raw = gen_raw(rng, 4001, 300, "tenth", ALL_NULLS)
    assert run_case(raw, build, [(1, abi.GT, PRED_CUT["half"])],
                    join_type=abi.ANTI, build_types=[I64],
                    anti_null_col=0) > 0


def test_fallback_two_keys():
    rng = np.random.default_rng(601)
    raw = gen_raw(rng, 4001, 300, "all", ALL_NULLS)
    bk = np.arange(300, dtype=np.int64) * 3 + 1
    build = [(np.tile(bk, 11), None),
             (np.repeat(np.arange(11, dtype=np.int64), 300), None)]
    projs = [(abi.PROJ_COPY, 0, -1), (abi.PROJ_COPY, 5, -1),
             (abi.PROJ_REV_F64, 2, 3)]
    assert run_case(raw, build, [(1, abi.GT, PRED_CUT["half"])],
                    keys=[EquiJoinKey(0, 0, I64), EquiJoinKey(1, 1, I64)],
                    projs=projs, out_types=[I64, I64, F64],
                    build_types=[I64, I64]) > 0


def test_fallback_residual_condition(small_build):
    rng = np.random.default_rng(602)
    raw = gen_raw(rng, 4001, 300, "all", ALL_NULLS)
    # condition row = outer cols then inner cols: inner payload (col 5) > 500
    assert run_case(raw, small_build, [(1, abi.GT, PRED_CUT["half"])],
                    conds=[JoinCond(5, abi.GT, -1, 500)]) > 0


def test_fallback_slice_projection(small_build):
    rng = np.random.default_rng(603)
    n = 2003
    raw = gen_raw(rng, n, 300, "all", ALL_NULLS)
    tags = [None if rng.random() < 0.05 else "t%d" % rng.integers(0, 50)
            for _ in range(n)]
    raw.append(Block.of(SLICE, tags))
    assert run_case(raw, small_build, [(1, abi.GT, PRED_CUT["half"])],
                    raw_types=RAW_TYPES + [SLICE],
                    projs=PROJS + [(abi.PROJ_COPY, 6, -1)],
                    out_types=OUT_TYPES + [SLICE]) > 0


# ---- errors: reported, never a fault ----

def test_errors(small_build):
    hip = abi.load_hip()
    rng = np.random.default_rng(700)
    raw = gen_raw(rng, 1000, 300, "all", ())
    ka = []
    gc = dev_chunk(hip, raw, RAW_TYPES, ka)
    s = ScanExec(hip, [(1, abi.GT, 49)], PROJS, RAW_TYPES, device=0)
    # projected types [I64, F64, I64, I32] vs probe side [I64, F64, I64, I64]
    bad = ParallelHashJoinExec(hip, abi.INNER, [EquiJoinKey(0, 0, I64)],
                               [I64, F64, I64, I64], BUILD_TYPES, device=0)
    good = ParallelHashJoinExec(hip, abi.INNER, [EquiJoinKey(0, 0, I64)],
                                OUT_TYPES, BUILD_TYPES, device=0)
    try:
        bad.consume_chunk(host_chunk(small_build, BUILD_TYPES))
        bad.build_consume()
        with pytest.raises(RuntimeError, match="types"):
            bad.probe_scan(s, C.byref(gc))
        good.consume_chunk(host_chunk(small_build, BUILD_TYPES))
        with pytest.raises(RuntimeError, match="probe before build"):
            good.probe_scan(s, C.byref(gc))
        # the ops stay usable after a reported error
        good.build_consume()
        out, kept = good.probe_scan(s, C.byref(gc))
        assert kept > 0 and out is not None
        assert hip.result_to_chunk(out).n_rows > 0
    finally:
        bad.close()
        good.close()
        s.close()
