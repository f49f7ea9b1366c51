"""Fused scan + group-join probe (gxop_groupjoin_probe_scan) parity.

Every case builds two group-joins from the same consumed rows on the HIP
library and compares, as multisets of emitted rows,
  (a) the fused call, raw chunk device-resident;
  (b) gxop_scan_consume then gxop_groupjoin_probe (the composed path);
  (c) where cheap, the CPU oracle's group-join over the numpy-filtered raw
      rows (the oracle's scan only projects them).
Integer columns and counts must be exact. The f64 inputs are small dyadic
rationals (k/8 prices, k/16 discounts), so every product and every partial
sum is exact, every summation order gives the same bits and f64 columns
compare with == as well; test_arbitrary_doubles_within_bound is the one
case with inexact sums. n_scan_kept and n_matched are checked against
numpy counts.
"""
import ctypes as C
from collections import Counter

import numpy as np
import pytest

from galaxysql_amd import abi
from galaxysql_amd.chunk import Block, Chunk, I64, I32, F64, SLICE, rows_of
from galaxysql_amd.operators import (HashGroupJoinExec, ScanExec, EquiJoinKey)

pytestmark = pytest.mark.gpu

# raw probe-side table
#   0 key i64, 1 date i32 (predicate column), 2 price f64, 3 disc f64,
#   4 cents i64, 5 disc hundredths i64, 6 cost i64, 7 qty i64
RAW_TYPES = [I64, I32, F64, F64, I64, I64, I64, I64]
PROJS = [(abi.PROJ_COPY, 0, -1), (abi.PROJ_REV_F64, 2, 3),
         (abi.PROJ_REV_SCALED4, 4, 5), (abi.PROJ_COPY, 1, -1),
         (abi.PROJ_Q9_AMOUNT4, 4, 5, 6, 7), (abi.PROJ_COPY, 2, -1)]
OUT_TYPES = [I64, F64, I64, I32, I64, F64]      # what PROJS produce
BUILD_TYPES = [I64, I32, I64]                   # key, i32 payload, i64 payload
Q3_AGGS = [(abi.SUM_F64, 1), (abi.SUM_I64, 2), (abi.COUNT_ROW, -1)]
KEYS = [EquiJoinKey(0, 0, I64)]
# the fused kernel's grid geometry (gxhip_scan.inc)
GX_PS_GRID_CAP = 4096
GX_PS_BLOCK_ROWS = 512


def gen_build(rng, n_keys, dup=1, key_nulls=False):
    keys = np.repeat(np.arange(n_keys, dtype=np.int64) * 3 + 1, dup)
    rng.shuffle(keys)
    n = len(keys)
    kn = None
    if key_nulls:
        kn = np.zeros(n, np.uint8)
        kn[:: max(n // 3, 1)] = 1
    return [(keys, kn),
            (rng.integers(0, 1000, n).astype(np.int32), None),
            (np.arange(n, dtype=np.int64), None)]


def gen_raw(rng, n, n_keys, match="tenth", null_cols=(), dyadic=True):
    span = max(n_keys, 1)
    if match == "none":
        key = rng.integers(0, span, n).astype(np.int64) * 3 + 2
    elif match == "all":
        key = rng.integers(0, span, n).astype(np.int64) * 3 + 1
    elif match == "one":
        key = np.full(n, 1, np.int64)
    else:
        key = rng.integers(0, 10 * span, n).astype(np.int64) * 3 + 1
    date = rng.integers(0, 100, n).astype(np.int32)
    cents = rng.integers(100, 1 << 20, n).astype(np.int64)
    disc = rng.integers(0, 11, n).astype(np.int64)
    if dyadic:
        price = cents.astype(np.float64) / 8.0
        fdisc = disc.astype(np.float64) / 16.0
    else:
        price = rng.random(n) * 1e5 + 1.0
        fdisc = rng.random(n) * 0.1
    vals = [key, date, price, fdisc, cents, disc,
            rng.integers(1, 1000, n).astype(np.int64),
            rng.integers(1, 50, n).astype(np.int64)]
    cols = []
    for c, v in enumerate(vals):
        nl = None
        if c in null_cols:
            nl = (rng.random(n) < 0.3).astype(np.uint8)
        cols.append((v, nl))
    return cols


def host_chunk(cols, types):
    return Chunk([c if isinstance(c, Block) else
                  Block(t, values=c[0], nulls=c[1])
                  for c, t in zip(cols, types)])


def dev_chunk(lib, cols, types, ka, lead=0):
    """GxChunk over device copies of the columns (mem = DEVICE). lead > 0
    uploads each array behind `lead` extra elements and passes the view
    past them: column pointers at odd element offsets."""
    import torch

    def up(a):
        a = np.array(a)
        if lead:
            a = np.concatenate([np.zeros(lead, a.dtype), a])
        t = torch.from_numpy(a).cuda()
        ka.append(t)
        v = t[lead:]
        return v.data_ptr() if v.numel() else None

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


def rows(chunks):
    return Counter(rows_of(chunks))


def n_rows_of(col):
    return col.n_rows if isinstance(col, Block) else len(col[0])


def pred_mask(raw_cols, preds):
    """numpy twin of the scan's predicates (date > cut; NULL fails)."""
    n = n_rows_of(raw_cols[0])
    m = np.ones(n, bool)
    for col, cmp, const in preds:
        assert cmp == abi.GT
        v, nl = raw_cols[col]
        m &= v > const
        if nl is not None:
            m &= nl == 0
    return m


def expected_matches(raw_cols, build_cols, mask, null_safe):
    """(survivor, consumed position) pairs with equal keys. The group-join
    matches NULL with NULL (null_safe) unless no consumed key is NULL."""
    bk, bn = build_cols[0]
    pk, pn = raw_cols[0]
    bnull = bn.astype(bool) if bn is not None else np.zeros(len(bk), bool)
    pnull = pn.astype(bool) if pn is not None else np.zeros(len(pk), bool)
    cnt = Counter(bk[~bnull].tolist())
    live = mask & ~pnull
    uk, uc = np.unique(pk[live], return_counts=True)
    total = sum(int(c) * cnt.get(int(k), 0) for k, c in zip(uk, uc))
    if null_safe:
        total += int((mask & pnull).sum()) * int(bnull.sum())
    return total


def take_rows(cols, types, mask):
    out = []
    for c, t in zip(cols, types):
        if isinstance(c, Block):
            vals = [c.get(i) for i in np.nonzero(mask)[0]]
            out.append(Block.of(SLICE, vals))
        else:
            out.append((c[0][mask], None if c[1] is None else c[1][mask]))
    return out


def run_case(raw_cols, build_cols, preds, *, aggs=Q3_AGGS, join_type=abi.INNER,
             keys=KEYS, raw_types=RAW_TYPES, projs=PROJS, out_types=OUT_TYPES,
             build_types=BUILD_TYPES, group_cols=(0, 1, 2), oracle=True,
             host_raw=False, lead=0, compare=True):
    """Returns (fused chunks, composed chunks, oracle chunks or None,
    fused stats dict, kept, matched)."""
    hip = abi.load_hip()
    assert hip.has_groupjoin_probe_scan
    group_cols = list(group_cols)
    build = host_chunk(build_cols, build_types)
    n_build = n_rows_of(build_cols[0])

    def make(lib, device):
        g = HashGroupJoinExec(lib, join_type, keys, build_types, out_types,
                              group_cols, aggs, device=device)
        if n_build:
            g.consume_chunk(build)
        g.build_consume()
        return g

    mask = pred_mask(raw_cols, preds)
    ref = None
    if oracle:
        orc = abi.load_oracle()
        assert not orc.has_groupjoin_probe_scan
        g = make(orc, -1)
        s = ScanExec(orc, [], projs, raw_types, device=-1)
        try:
            if mask.any():
                t = s.consume_chunk(host_chunk(
                    take_rows(raw_cols, raw_types, mask), raw_types))
                g.probe_chunk(t)
            ref = g.result_chunks()
        finally:
            g.close()
            s.close()

    ga, gb = make(hip, 0), make(hip, 0)
    s = ScanExec(hip, preds, projs, raw_types, device=0)
    try:
        ka = []
        if host_raw:
            gc = hip.to_gx_chunk(host_chunk(raw_cols, raw_types), ka)
        else:
            gc = dev_chunk(hip, raw_cols, raw_types, ka, lead=lead)
        # (a) fused
        kept, matched = ga.probe_scan(s, C.byref(gc))
        stats = ga.stats()
        got_a = ga.result_chunks()
        # (b) composed, on an op built from the same data
        t = s.consume_raw(C.byref(gc))
        kept_b = t.contents.chunk.n_rows
        hip.check(hip.lib.gxop_groupjoin_probe(gb._op,
                                               C.byref(t.contents.chunk)),
                  "groupjoin_probe")
        hip.lib.gxop_result_release(t)
        stats_b = gb.stats()
        got_b = gb.result_chunks()
    finally:
        ga.close()
        gb.close()
        s.close()

    bn = build_cols[0][1] if not isinstance(build_cols[0], Block) else None
    null_safe = bn is not None and bool(np.any(bn))
    want_kept = int(mask.sum())
    want_matched = expected_matches(raw_cols, build_cols, mask, null_safe) \
        if len(keys) == 1 else None
    n_out = sum(c.n_rows for c in got_a)
    print(f"kept fused/composed/numpy = {kept}/{kept_b}/{want_kept}, "
          f"matched fused/composed/numpy = {matched}/{stats_b['matches']}/"
          f"{want_matched}, rows = {n_out}")
    assert kept == kept_b == want_kept
    assert matched == stats_b["matches"]
    if want_matched is not None:
        assert matched == want_matched
    if compare:
        assert rows(got_a) == rows(got_b), "fused != composed"
        if ref is not None:
            assert rows(got_b) == rows(ref), "composed != oracle"
            assert rows(got_a) == rows(ref), "fused != oracle"
    return got_a, got_b, ref, stats, kept, matched


HALF = [(1, abi.GT, 49)]
ALL = [(1, abi.GT, -1)]
NONE = [(1, abi.GT, 1000)]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 127, 128, 129, 511, 513])
def test_tile_and_wave_edges(n):
    rng = np.random.default_rng(n)
    run_case(gen_raw(rng, n, 20, match="all"), gen_build(rng, 20), HALF)


def test_grid_carry_over():
    """Just past one full grid pass: the waves of the first blocks run a
    second grid-stride iteration with queue entries carried over."""
    rng = np.random.default_rng(1)
    n = GX_PS_GRID_CAP * GX_PS_BLOCK_ROWS + 300
    got, _, _, _, kept, matched = run_case(
        gen_raw(rng, n, 300), gen_build(rng, 300), HALF, oracle=False)
    assert kept > 0 and matched > 0 and sum(c.n_rows for c in got) == 300


def test_full_survival_overflows_the_stage():
    rng = np.random.default_rng(2)
    got, *_ = run_case(gen_raw(rng, 5000, 500, match="all"),
                       gen_build(rng, 500), ALL)
    assert sum(c.n_rows for c in got) == 500


def test_bloom_sized_build():
    """>= 65536 consumed rows: the size from which the inline-bucket build
    adds the bloom filter the kernel tests before the walk."""
    rng = np.random.default_rng(20)
    run_case(gen_raw(rng, 30_000, 70_000), gen_build(rng, 70_000), HALF,
             oracle=False)


def test_overflow_runs_six_duplicates():
    """Build keys 6x: runs past the 4 inline slots; each probe row
    accumulates into all 6 positions, 6 groups per key are emitted."""
    rng = np.random.default_rng(3)
    raw = gen_raw(rng, 3000, 40, match="all")
    got, _, _, _, kept, matched = run_case(raw, gen_build(rng, 40, dup=6),
                                           ALL)
    assert kept == 3000 and matched == 6 * 3000
    per_key = Counter(r[0] for r in rows_of(got))
    assert set(per_key.values()) == {6}
    by_pos = {}
    for r in rows_of(got):
        by_pos.setdefault(r[0], set()).add(r[3:])
    assert all(len(v) == 1 for v in by_pos.values())  # 6 equal accumulations


def test_hot_group():
    rng = np.random.default_rng(4)
    n = 100_000
    raw = gen_raw(rng, n, 10, match="one")
    got, *_ = run_case(raw, gen_build(rng, 10), ALL)
    (r,) = rows_of(got)
    cents, disc = raw[4][0], raw[5][0]
    assert r[4] == int((cents * (100 - disc)).sum()) and r[5] == n


@pytest.mark.parametrize("what", ["no_match", "empty_build", "no_survivor"])
def test_nothing_to_emit(what):
    rng = np.random.default_rng(5)
    raw = gen_raw(rng, 700, 50, match="none" if what == "no_match" else "all")
    build = gen_build(rng, 0 if what == "empty_build" else 50)
    preds = NONE if what == "no_survivor" else HALF
    got, _, _, _, kept, matched = run_case(raw, build, preds)
    assert matched == 0 and sum(c.n_rows for c in got) == 0
    assert (kept == 0) == (what == "no_survivor")


def test_null_probe_keys_match_nothing():
    rng = np.random.default_rng(6)
    raw = gen_raw(rng, 2000, 30, match="all", null_cols=(0,))
    _, _, _, _, kept, matched = run_case(raw, gen_build(rng, 30), ALL)
    assert matched == int((raw[0][1] == 0).sum()) < kept


def test_null_agg_inputs():
    """COUNT_COL skips NULL inputs; a SUM_F64 group whose only inputs are
    NULL comes out NULL."""
    rng = np.random.default_rng(7)
    raw = gen_raw(rng, 1500, 12, match="all", null_cols=(2, 4))
    price_n = raw[2][1]
    price_n[raw[0][0] == 1] = 1         # every price of key 1 is NULL
    aggs = [(abi.COUNT_COL, 1), (abi.SUM_F64, 1), (abi.COUNT_COL, 2),
            (abi.SUM_I64, 2), (abi.COUNT_ROW, -1)]
    got, *_ = run_case(raw, gen_build(rng, 12), ALL, aggs=aggs)
    r = [x for x in rows_of(got) if x[0] == 1]
    assert len(r) == 1 and r[0][3] == 0 and r[0][4] is None and r[0][7] > 0


def test_null_consumed_key_takes_the_csr_path():
    rng = np.random.default_rng(8)
    raw = gen_raw(rng, 2000, 30, match="all", null_cols=(0,))
    build = gen_build(rng, 30, key_nulls=True)
    _, _, _, _, _, matched = run_case(raw, build, ALL)
    # null-safe matching there: NULL probe keys met the NULL consumed keys
    assert matched > expected_matches(raw, build, pred_mask(raw, ALL), False)


def test_left_emits_unmatched_positions():
    rng = np.random.default_rng(9)
    raw = gen_raw(rng, 400, 200)        # ~1 in 10 keys present
    got, *_ = run_case(raw, gen_build(rng, 200), HALF, join_type=abi.LEFT,
                       aggs=Q3_AGGS + [(abi.COUNT_COL, 2)])
    out = rows_of(got)
    assert len(out) == 200
    unmatched = [r for r in out if r[3] is None]
    assert unmatched and all(r[4] == 0 and r[5] == 1 and r[6] == 0
                             for r in unmatched)


def test_every_aggregate_over_projections():
    rng = np.random.default_rng(10)
    raw = gen_raw(rng, 4000, 25, match="all", null_cols=(1, 3, 6))
    aggs = [(abi.MIN_I64, 3), (abi.MAX_I64, 3),        # I32 COPY
            (abi.MIN_F64, 1), (abi.MAX_F64, 1),        # REV_F64
            (abi.AVG_F64, 5), (abi.SUM_F64, 3),        # F64 COPY, I32 COPY
            (abi.BIT_AND, 3), (abi.BIT_OR, 2), (abi.BIT_XOR, 4),
            (abi.MAX_I64, 4), (abi.MIN_I64, 4),        # Q9_AMOUNT4
            (abi.SUM_I64, 3), (abi.COUNT_COL, 4), (abi.COUNT_ROW, -1)]
    build = gen_build(rng, 25)
    run_case(raw, build, [(7, abi.GT, 10)], aggs=aggs)
    # SUM_I64N: the oracle's group-join has no case for it (its state stays
    # NULL), so this one is fused against composed only
    got, *_ = run_case(raw, build, [(7, abi.GT, 10)], oracle=False,
                       aggs=[(abi.SUM_I64N, 4), (abi.SUM_I64N, 3),
                             (abi.SUM_I64, 4), (abi.COUNT_COL, 4)])
    assert all((r[3] is None) == (r[6] == 0) and
               (r[3] is None or r[3] == r[5]) for r in rows_of(got))


def test_unaligned_views():
    rng = np.random.default_rng(11)
    run_case(gen_raw(rng, 1000, 30, match="all", null_cols=(4,)),
             gen_build(rng, 30), HALF, lead=1)
    run_case(gen_raw(rng, 1000, 30, match="all"), gen_build(rng, 30), HALF,
             lead=3, oracle=False)


def test_fallback_two_key_join():
    rng = np.random.default_rng(12)
    raw = gen_raw(rng, 1500, 20, match="all")
    build = gen_build(rng, 20, dup=3)
    build[1] = (rng.integers(0, 100, 60).astype(np.int32), None)
    run_case(raw, build, HALF,
             keys=[EquiJoinKey(0, 0, I64), EquiJoinKey(1, 3, I32)])


def test_fallback_host_chunk():
    rng = np.random.default_rng(13)
    run_case(gen_raw(rng, 900, 20, match="all"), gen_build(rng, 20), HALF,
             host_raw=True)


def test_fallback_wide_mode_aggregates():
    """<= 2 aggregates of COUNT/SUM_I64 keep the CSR wide mode: composed."""
    rng = np.random.default_rng(14)
    run_case(gen_raw(rng, 900, 20, match="all"), gen_build(rng, 20), HALF,
             aggs=[(abi.SUM_I64, 2), (abi.COUNT_ROW, -1)])


def slice_col(rng, n, nulls=False):
    vals = [f"s{int(x)}" for x in rng.integers(0, 50, n)]
    if nulls:
        vals = [None if i % 7 == 0 else v for i, v in enumerate(vals)]
    return Block.of(SLICE, vals)


def test_fallback_slice_agg_input():
    rng = np.random.default_rng(15)
    n = 800
    raw = gen_raw(rng, n, 20, match="all") + [slice_col(rng, n, nulls=True)]
    run_case(raw, gen_build(rng, 20), HALF, raw_types=RAW_TYPES + [SLICE],
             projs=PROJS + [(abi.PROJ_COPY, 8, -1)],
             out_types=OUT_TYPES + [SLICE],
             aggs=Q3_AGGS + [(abi.COUNT_COL, 6)])


def test_slice_group_column_keeps_the_per_column_emission():
    rng = np.random.default_rng(16)
    build = gen_build(rng, 20) + [slice_col(rng, 20)]
    run_case(gen_raw(rng, 800, 20, match="all"), build, HALF,
             build_types=BUILD_TYPES + [SLICE], group_cols=(0, 3, 1))


@pytest.mark.parametrize("join_type", [abi.INNER, abi.LEFT])
def test_one_kernel_emission(join_type):
    """I64 and I32 group columns, the rows the oracle emits; null-free
    blocks come back without a nulls array (gxop_result_to_host accepted
    them: result_chunks went through it)."""
    rng = np.random.default_rng(17)
    build = gen_build(rng, 150)
    got, comp, _, _, _, _ = run_case(
        gen_raw(rng, 600, 150), build, HALF, join_type=join_type,
        aggs=Q3_AGGS + [(abi.AVG_F64, 5)], group_cols=(2, 1, 0))
    for chunks in (got, comp):
        for ch in chunks:
            b = ch.blocks
            assert all(x.nulls is None for x in b[:3])      # key columns
            assert b[4].nulls is None and b[5].nulls is None  # SUM_I64, COUNT
            assert b[3].nulls is not None and b[6].nulls is not None
    # a consumed column that carries NULLs keeps its nulls array
    build[1] = (build[1][0], (np.arange(150) % 5 == 0).astype(np.uint8))
    got, *_ = run_case(gen_raw(rng, 600, 150), build, HALF,
                       join_type=join_type, group_cols=(2, 1, 0))
    assert all(ch.blocks[1].nulls is not None for ch in got)


def test_stats():
    rng = np.random.default_rng(18)
    _, _, _, st, kept, matched = run_case(
        gen_raw(rng, 5000, 100, match="all"), gen_build(rng, 100), HALF)
    assert st["probe_rows"] == kept > 0 and st["matches"] == matched > 0
    assert st["probe_launches"] == 1 and st["probe_kernel_ms"] > 0.0


def test_arbitrary_doubles_within_bound():
    """Inexact sums: any two summation orders of m positive terms differ by
    at most (m - 1) * 2^-52 relative, the bound the project uses."""
    rng = np.random.default_rng(19)
    raw = gen_raw(rng, 20_000, 40, match="all", dyadic=False)
    got, comp, ref, *_ = run_case(raw, gen_build(rng, 40), ALL, compare=False)

    def table(chunks):
        return {r[:3]: r[3:] for r in rows_of(chunks)}

    a, b, c = table(got), table(comp), table(ref)
    assert a.keys() == b.keys() == c.keys() and len(a) == 40
    bound = (max(v[2] for v in c.values()) - 1) * 2.0 ** -52
    worst = 0.0
    for k, (fsum, isum, cnt) in c.items():
        for other in (a[k], b[k]):
            assert other[1:] == (isum, cnt)
            worst = max(worst, abs(other[0] - fsum) / fsum)
    print(f"worst relative difference {worst:.3e}, bound {bound:.3e}")
    assert worst <= bound
