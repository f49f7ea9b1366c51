"""A producer join's matches straight into a group-join's build
(gxop_groupjoin_build_probe_scan) parity.

Every case runs one producer join (join1: customer build, probed with an
unscanned orders table) into two group-joins on the HIP library:
  (a) gxop_groupjoin_build_probe_scan;
  (b) gxop_join_probe_scan -> gxop_groupjoin_consume -> gxop_groupjoin_build.
Both are then probed with the same lineitem chunk and their emitted rows
compared as multisets (consumed positions, hence row order, are undefined).
Integer columns are exact; the f64 inputs are dyadic (k/8), so every sum is
exact in any order and f64 columns compare with == too. n_scan_kept and
n_consumed are checked against numpy, and where cheap the emission against
the CPU oracle's group-join over the numpy-filtered orders rows.
gxop_groupjoin_build_was_fused tells which path (a) took, so a case that
means the one-kernel path cannot pass through the composed one unnoticed.
"""
import ctypes as C

import numpy as np
import pytest

from galaxysql_amd import abi
from galaxysql_amd.chunk import Block, I64, I32, F64, SLICE
from galaxysql_amd.operators import (HashGroupJoinExec, ParallelHashJoinExec,
                                     ScanExec, EquiJoinKey)

from .test_gpu_groupjoin_probe_scan import (dev_chunk, host_chunk, take_rows,
                                            pred_mask, slice_col)

pytestmark = pytest.mark.gpu

# raw orders: 0 custkey i64 (join1's probe key), 1 orderkey i64 (the
# group-join's consumed key), 2 date i32 (predicate column), 3 prio i32,
# 4 value f64 (dyadic)
ORD_TYPES = [I64, I64, I32, I32, F64]
CUST_TYPES = [I64, I32]                       # custkey, segment
LI_TYPES = [I64, F64, I64]                    # orderkey, revenue, cents
Q3_AGGS = [(abi.SUM_F64, 1), (abi.SUM_I64, 2), (abi.COUNT_ROW, -1)]
MINMAX_AGGS = [(abi.MIN_I64, 2), (abi.MAX_F64, 1), (abi.MIN_F64, 1),
               (abi.COUNT_COL, 1)]
ALL = [(2, abi.GT, -1)]
HALF = [(2, abi.GT, 49)]
NONE = [(2, abi.GT, 1000)]
N_CUST = 300


def copy_projs(n):
    return [(abi.PROJ_COPY, c, -1) for c in range(n)]


def gen_cust(rng, n=N_CUST):
    return [(np.arange(n, dtype=np.int64), None),
            (rng.integers(0, 5, n).astype(np.int32), None)]


def gen_orders(rng, n_raw, n_match, dup=1, null_cols=()):
    """n_raw rows of which exactly n_match carry a custkey the customer
    table holds; orderkeys unique, or `dup` rows per orderkey."""
    ck = np.full(n_raw, N_CUST + 11, np.int64)
    ck[:n_match] = rng.integers(0, N_CUST, n_match)
    rng.shuffle(ck)
    ok = np.repeat(np.arange((n_raw + dup - 1) // dup, dtype=np.int64),
                   dup)[:n_raw] * 3 + 1
    rng.shuffle(ok)
    vals = [ck, ok, rng.integers(0, 100, n_raw).astype(np.int32),
            rng.integers(0, 3, n_raw).astype(np.int32),
            rng.integers(0, 1 << 20, n_raw).astype(np.float64) / 8.0]
    cols = []
    for c, v in enumerate(vals):
        nl = (rng.random(n_raw) < 0.3).astype(np.uint8) \
            if c in null_cols else None
        cols.append((v, nl))
    return cols


def gen_li(rng, n, orders):
    """probe rows for the group-join: about half hit an orderkey"""
    ok = orders[1][0]
    key = np.where(rng.random(n) < 0.5,
                   ok[rng.integers(0, max(len(ok), 1), n)] if len(ok)
                   else np.full(n, 2, np.int64),
                   rng.integers(0, 1000, n).astype(np.int64) * 3 + 2)
    cents = rng.integers(100, 1 << 20, n).astype(np.int64)
    return [(key.astype(np.int64), None),
            (cents.astype(np.float64) / 8.0, None), (cents, None)]


def canon(chunks):
    """rows as a lexsorted int64 matrix (value bits with NULLs zeroed, then
    the null flag, per column): equal matrices = equal row multisets"""
    chunks = [c for c in chunks if c.n_rows]
    if not chunks:
        return np.zeros((0, 0), np.int64)
    cols = []
    for ci in range(len(chunks[0].blocks)):
        v = np.concatenate([np.ascontiguousarray(c.blocks[ci].values)
                            for c in chunks])
        nl = np.concatenate([
            c.blocks[ci].nulls if c.blocks[ci].nulls is not None
            else np.zeros(c.n_rows, np.uint8) for c in chunks]).astype(np.int64)
        v = v.view(np.int64) if v.dtype == np.float64 else v.astype(np.int64)
        cols += [np.where(nl == 1, 0, v), nl]
    m = np.stack(cols)
    return m[:, np.lexsort(m[::-1])]


def same_rows(a, b):
    ca, cb = canon(a), canon(b)
    return ca.shape == cb.shape and np.array_equal(ca, cb)


def n_rows(chunks):
    return sum(c.n_rows for c in chunks)


def run_case(orders, cust, li, preds, *, j1_type=abi.SEMI, out_proj=None,
             aggs=Q3_AGGS, gj_type=abi.INNER, group_cols=(1, 2, 3),
             ord_types=ORD_TYPES, expect_fused=True, host_raw=False, lead=0,
             pre=None, li_scan=False, oracle=True):
    """Returns (rows of (a), rows of (b), kept, consumed)."""
    hip = abi.load_hip()
    assert hip.has_groupjoin_build_probe_scan
    group_cols = list(group_cols)
    if j1_type == abi.SEMI:
        consumed_types = list(ord_types)
    else:
        full = list(ord_types) + CUST_TYPES
        consumed_types = [full[i] for i in out_proj] if out_proj else full
    keys = [EquiJoinKey(1, 0, I64)]

    mask = pred_mask(orders, preds)
    ckn = orders[0][1]
    mask &= np.isin(orders[0][0], cust[0][0])
    if ckn is not None:
        mask &= ckn == 0

    j1 = ParallelHashJoinExec(hip, j1_type, [EquiJoinKey(0, 0, I64)],
                              outer_types=ord_types, inner_types=CUST_TYPES,
                              device=0, out_proj=out_proj, enable_bloom=True)
    so = ScanExec(hip, preds, copy_projs(len(ord_types)), ord_types, device=0)
    ga = HashGroupJoinExec(hip, gj_type, keys, consumed_types, LI_TYPES,
                           group_cols, aggs, device=0)
    gb = HashGroupJoinExec(hip, gj_type, keys, consumed_types, LI_TYPES,
                           group_cols, aggs, device=0)
    sl = None
    try:
        j1.consume_chunk(host_chunk(cust, CUST_TYPES))
        j1.build_consume()
        if pre is not None:
            ga.consume_chunk(host_chunk(pre, consumed_types))
            gb.consume_chunk(host_chunk(pre, consumed_types))
        ka = []
        if host_raw:
            gc = hip.to_gx_chunk(host_chunk(orders, ord_types), ka)
        else:
            gc = dev_chunk(hip, orders, ord_types, ka, lead=lead)
        # (a) the new entry
        kept, consumed = ga.build_probe_scan(j1, so, C.byref(gc))
        fused = ga.build_was_fused()
        # (b) the composed sequence
        r, kept_b = j1.probe_scan(so, C.byref(gc))
        consumed_b = 0
        if r:
            consumed_b = r.contents.chunk.n_rows
            hip.check(hip.lib.gxop_groupjoin_consume(
                gb._op, C.byref(r.contents.chunk)), "groupjoin_consume")
            hip.lib.gxop_result_release(r)
        gb.build_consume()
        assert not gb.build_was_fused()
        # probe both alike
        if li_scan:
            raw_li = li + [(np.arange(len(li[0][0]), dtype=np.int32) % 100,
                            None)]
            sl = ScanExec(hip, [(3, abi.GT, 49)], copy_projs(3),
                          LI_TYPES + [I32], device=0)
            lgc = dev_chunk(hip, raw_li, LI_TYPES + [I32], ka)
            ga.probe_scan(sl, C.byref(lgc))
            gb.probe_scan(sl, C.byref(lgc))
        elif len(li[0][0]):
            ga.probe_chunk(host_chunk(li, LI_TYPES))
            gb.probe_chunk(host_chunk(li, LI_TYPES))
        got_a, got_b = ga.result_chunks(), gb.result_chunks()
    finally:
        for op in (ga, gb, j1, so, sl):
            if op is not None:
                op.close()

    want_kept = int(pred_mask(orders, preds).sum())
    want_consumed = int(mask.sum())
    print(f"kept new/composed/numpy = {kept}/{kept_b}/{want_kept}, consumed "
          f"new/composed/numpy = {consumed}/{consumed_b}/{want_consumed}, "
          f"fused = {fused}, rows = {n_rows(got_a)}/{n_rows(got_b)}")
    assert kept == kept_b == want_kept
    assert consumed == consumed_b == want_consumed
    # an empty consumed side builds nothing either way
    assert fused == (expect_fused and want_consumed > 0)
    assert same_rows(got_a, got_b), "new entry != composed"

    if oracle and j1_type == abi.SEMI and pre is None and not li_scan:
        orc = abi.load_oracle()
        assert not orc.has_groupjoin_build_probe_scan
        g = HashGroupJoinExec(orc, gj_type, keys, consumed_types, LI_TYPES,
                              group_cols, aggs, device=-1)
        try:
            if mask.any():
                g.consume_chunk(host_chunk(take_rows(orders, ord_types, mask),
                                           ord_types))
            g.build_consume()
            if len(li[0][0]):
                g.probe_chunk(host_chunk(li, LI_TYPES))
            ref = g.result_chunks()
        finally:
            g.close()
        assert same_rows(got_b, ref), "composed != oracle"
        assert same_rows(got_a, ref), "new entry != oracle"
    return got_a, got_b, kept, consumed


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_consumed_row_counts(n):
    rng = np.random.default_rng(n)
    orders = gen_orders(rng, n + 37, n)
    got, _, _, consumed = run_case(orders, gen_cust(rng),
                                   gen_li(rng, 4 * n + 50, orders), ALL,
                                   gj_type=abi.LEFT)
    assert consumed == n and n_rows(got) == n   # LEFT: every position


@pytest.mark.parametrize("why", ["predicate", "join"])
def test_nothing_consumed(why):
    rng = np.random.default_rng(100)
    orders = gen_orders(rng, 500, 200 if why == "predicate" else 0)
    for gj_type in (abi.INNER, abi.LEFT):
        got, _, kept, consumed = run_case(
            orders, gen_cust(rng), gen_li(rng, 300, orders),
            NONE if why == "predicate" else ALL, gj_type=gj_type)
        assert consumed == 0 and n_rows(got) == 0
        assert (kept == 0) == (why == "predicate")


def test_second_grid_pass():
    """1,048,576 + 65 consumed rows: the first blocks of the 4096 x 256 grid
    run a second grid-stride iteration. LEFT, so every consumed row is
    emitted and compared."""
    rng = np.random.default_rng(101)
    n = (1 << 20) + 65
    orders = gen_orders(rng, n + 500, n)
    got, _, _, consumed = run_case(orders, gen_cust(rng),
                                   gen_li(rng, 20_000, orders), ALL,
                                   gj_type=abi.LEFT, oracle=False)
    assert consumed == n and n_rows(got) == n


@pytest.mark.parametrize("gj_type", [abi.INNER, abi.LEFT])
def test_six_duplicates_per_key_spill(gj_type):
    """Ranks >= 4 of a bucket go through the spill list; the group-join
    emits one group per consumed position."""
    rng = np.random.default_rng(102)
    orders = gen_orders(rng, 1200, 1200, dup=6)
    got, _, _, consumed = run_case(orders, gen_cust(rng),
                                   gen_li(rng, 3000, orders), ALL,
                                   gj_type=gj_type)
    assert consumed == 1200
    if gj_type == abi.LEFT:
        keys = np.concatenate([c.blocks[0].values for c in got])
        assert set(np.unique(keys, return_counts=True)[1].tolist()) == {6}


def test_inner_producer_with_a_build_side_column():
    """join1 INNER, out_proj keeping the customer's segment: a consumed
    column gathered at the build position."""
    rng = np.random.default_rng(103)
    orders = gen_orders(rng, 2000, 900)
    got, *_ = run_case(orders, gen_cust(rng), gen_li(rng, 4000, orders), HALF,
                       j1_type=abi.INNER, out_proj=[0, 1, 2, 3, 4, 6],
                       group_cols=(1, 5, 2))
    assert n_rows(got) > 0


def test_min_max_aggregates():
    rng = np.random.default_rng(104)
    orders = gen_orders(rng, 1500, 800)
    got, *_ = run_case(orders, gen_cust(rng), gen_li(rng, 5000, orders), HALF,
                       aggs=MINMAX_AGGS)
    assert n_rows(got) > 0


def test_probed_through_the_fused_probe_scan():
    rng = np.random.default_rng(105)
    orders = gen_orders(rng, 3000, 1500)
    got, *_ = run_case(orders, gen_cust(rng), gen_li(rng, 8000, orders), HALF,
                       li_scan=True)
    assert n_rows(got) > 0


def test_bloom_sized_build():
    """>= 65536 consumed rows: the build also sets the bloom bits the
    group-join's probe-scan tests."""
    rng = np.random.default_rng(106)
    orders = gen_orders(rng, 80_000, 70_000)
    got, _, _, consumed = run_case(orders, gen_cust(rng),
                                   gen_li(rng, 30_000, orders), ALL,
                                   li_scan=True, oracle=False)
    assert consumed == 70_000 and n_rows(got) > 0


def test_i32_and_f64_group_columns_with_nulls():
    """a non-key consumed column with a nulls buffer: its nulls arrive"""
    rng = np.random.default_rng(107)
    orders = gen_orders(rng, 1500, 900, null_cols=(2, 4))
    got, _, _, _ = run_case(orders, gen_cust(rng), gen_li(rng, 6000, orders),
                            ALL, group_cols=(1, 2, 4), gj_type=abi.LEFT)
    b = [np.concatenate([c.blocks[i].nulls for c in got]) for i in (1, 2)]
    want = pred_mask(orders, ALL) & np.isin(orders[0][0], np.arange(N_CUST))
    # the predicate column's NULL rows fail the predicate; the f64 column's
    # NULLs among the consumed rows all arrive
    assert int(b[0].sum()) == 0
    assert int(b[1].sum()) == int(orders[4][1][want].sum()) > 0


def test_unaligned_views():
    rng = np.random.default_rng(108)
    orders = gen_orders(rng, 1000, 600, null_cols=(4,))
    run_case(orders, gen_cust(rng), gen_li(rng, 3000, orders), HALF, lead=1)


def test_fallback_null_raw_key_column():
    rng = np.random.default_rng(109)
    orders = gen_orders(rng, 1000, 600, null_cols=(1,))
    run_case(orders, gen_cust(rng), gen_li(rng, 3000, orders), HALF,
             expect_fused=False)


def test_fallback_slice_column():
    rng = np.random.default_rng(110)
    n = 800
    orders = gen_orders(rng, n, 500) + [slice_col(rng, n, nulls=True)]
    run_case(orders, gen_cust(rng), gen_li(rng, 2000, orders), HALF,
             ord_types=ORD_TYPES + [SLICE], expect_fused=False, oracle=False)


def test_fallback_host_chunk():
    rng = np.random.default_rng(111)
    orders = gen_orders(rng, 900, 500)
    run_case(orders, gen_cust(rng), gen_li(rng, 2000, orders), HALF,
             host_raw=True, expect_fused=False)


def test_fallback_op_that_already_consumed():
    rng = np.random.default_rng(112)
    orders = gen_orders(rng, 900, 500)
    pre_keys = np.arange(40, dtype=np.int64) * 3 + 2      # no orders key
    pre = [(np.zeros(40, np.int64), None), (pre_keys, None),
           (np.full(40, 7, np.int32), None), (np.zeros(40, np.int32), None),
           (np.full(40, 0.5), None)]
    got, _, _, consumed = run_case(orders, gen_cust(rng),
                                   gen_li(rng, 2000, orders), ALL, pre=pre,
                                   gj_type=abi.LEFT, expect_fused=False)
    keys = np.concatenate([c.blocks[0].values for c in got])
    assert len(keys) == 40 + consumed and np.isin(pre_keys, keys).all()


def test_switch_off_equals_default(monkeypatch):
    rng = np.random.default_rng(113)
    orders = gen_orders(rng, 2000, 1200)
    cust, li = gen_cust(rng), gen_li(rng, 5000, orders)
    on, *_ = run_case(orders, cust, li, HALF)
    monkeypatch.setenv("GX_GJ_BUILD_FUSED", "0")
    off, *_ = run_case(orders, cust, li, HALF, expect_fused=False)
    assert same_rows(on, off)


def test_q3_plan_with_the_switch_on_and_off(monkeypatch):
    import torch
    from galaxysql_amd.queries import run_q3_honest, gen_q3_raw_numpy
    hip = abi.load_hip()
    data = gen_q3_raw_numpy(np.random.default_rng(114), n_cust=600,
                            n_orders=5000, n_lineitem=20000)
    t = [[torch.from_numpy(a).cuda() for a in cols] for cols in data]

    def go():
        chunks, info = run_q3_honest(hip, 0, t[0], t[1], t[2], to_host=True)
        return chunks, info

    on, info_on = go()
    monkeypatch.setenv("GX_GJ_BUILD_FUSED", "0")
    off, info_off = go()
    for k in ("cust_kept", "orders_kept_scan", "lineitem_kept",
              "orders_kept", "joined_rows", "groups"):
        print(k, info_on[k], info_off[k])
        assert info_on[k] == info_off[k], k
    assert info_on["groups"] == n_rows(on) > 0
    # revenue sums are not dyadic here: integer columns exact, the f64 sum
    # within (max COUNT - 1) * 2^-52 relative of the other order's
    a, b = canon(on), canon(off)
    assert a.shape == b.shape
    keep = [r for r in range(a.shape[0]) if r != 6]   # 6 = SUM f64 bits
    oa = a[:, np.lexsort(a[keep][::-1])]
    ob = b[:, np.lexsort(b[keep][::-1])]
    assert np.array_equal(oa[keep], ob[keep])
    fa, fb = oa[6].view(np.float64), ob[6].view(np.float64)
    bound = (int(oa[10].max()) - 1) * 2.0 ** -52
    worst = float(np.max(np.abs(fa - fb) / np.abs(fb)))
    print(f"worst relative difference {worst:.3e}, bound {bound:.3e}")
    assert worst <= bound
