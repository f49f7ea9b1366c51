"""Device sort / top-N (gxop_sort_*: SortExec, TopNExec) against the CPU
reference of tests/sort_ref.py. Device output must equal the reference as an
exact row SEQUENCE (the operator is stable); F64 compares by bit pattern,
NaN-canonicalised on order columns only, so payload NaNs must come back
bit-identical. Shapes are the smallest that reach each path: wave and block
edges, a grid-stride second and third trip, both top-N paths (forced with
GX_TOPN_SELECT and proven by the stats), every select exit, compaction."""
import ctypes as C
import os

import numpy as np
import pytest

from galaxysql_amd import abi
from galaxysql_amd.chunk import (Block, Chunk, I64, I32, F64, SLICE, DECIMAL,
                                 chunks_from_columns, dec40_encode)
from galaxysql_amd.operators import OrderByOption, SortExec, TopNExec

from . import sort_ref as sr

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
SELECT_SLACK = 1 << 16   # the select stops refining at max(4K, 64Ki) rows


@pytest.fixture(scope="module")
def hip():
    return abi.load_hip()


class select_mode:
    """GX_TOPN_SELECT for ops created inside: '0', '1' or None (gate)."""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        self.old = os.environ.pop("GX_TOPN_SELECT", None)
        if self.mode is not None:
            os.environ["GX_TOPN_SELECT"] = str(self.mode)

    def __exit__(self, *a):
        os.environ.pop("GX_TOPN_SELECT", None)
        if self.old is not None:
            os.environ["GX_TOPN_SELECT"] = self.old


def run_device(hip, types, chunks, order, offset=0, fetch=-1, select=None,
               null_last=False, **kw):
    """-> ([(values, nulls)] per column, stats, result chunks)."""
    obs = [OrderByOption(c, a, null_last) for c, a in order]
    with select_mode(select):
        op = SortExec(hip, obs, types, offset=offset, fetch=fetch, device=0,
                      **kw)
    try:
        for ch in chunks:
            op.consume_chunk(ch)
        op.build_consume()
        out = op.result_chunks()
        st = op.stats()
    finally:
        op.close()
    return sr.concat_columns(out, types), st, out


def assert_columns_equal(got, exp, types, order):
    order_cols = {c for c, _ in order}
    for ci, ((gv, gn), (ev, en)) in enumerate(zip(got, exp)):
        assert len(gn) == len(en), f"col {ci}: {len(gn)} rows, want {len(en)}"
        assert np.array_equal(gn != 0, en != 0), f"col {ci} nulls differ"
        live = en == 0
        if isinstance(ev, list):
            assert [v for v, l in zip(gv, live) if l] == \
                   [v for v, l in zip(ev, live) if l], f"col {ci}"
            continue
        if types[ci] == F64:
            gb, eb = sr.f64_bits(gv).copy(), sr.f64_bits(ev).copy()
            if ci in order_cols:
                gb[np.isnan(gv)] = sr.CANON_NAN
                eb[np.isnan(ev)] = sr.CANON_NAN
            gv, ev = gb, eb
        bad = np.flatnonzero((gv != ev) & live)
        assert bad.size == 0, (f"col {ci}: first mismatch at output row "
                               f"{bad[0]}: {gv[bad[0]]} != {ev[bad[0]]}")


def check(hip, types, chunks, order, offset=0, fetch=-1, select=None,
          cols=None, perm=None, **kw):
    """Device == reference, as a sequence. cols/perm: a precomputed
    reference order shared between calls."""
    if cols is None:
        cols = sr.concat_columns(chunks, types)
    if perm is None:
        perm = sr.sort_perm(cols, types, order)
    exp = sr.gather_columns(cols, sr.limit(perm, offset, fetch))
    got, st, out = run_device(hip, types, chunks, order, offset, fetch,
                              select, **kw)
    assert_columns_equal(got, exp, types, order)
    return st, out


def both_paths(hip, types, chunks, order, fetch, offset=0, **kw):
    """The same bounded query through the forced select and the forced full
    sort; both equal the reference. Returns the select run's stats."""
    cols = sr.concat_columns(chunks, types)
    perm = sr.sort_perm(cols, types, order)
    n = len(perm)
    s0, _ = check(hip, types, chunks, order, offset, fetch, select=0,
                  cols=cols, perm=perm, **kw)
    assert not s0["used_select"] and s0["select_passes"] == 0
    s1, _ = check(hip, types, chunks, order, offset, fetch, select=1,
                  cols=cols, perm=perm, **kw)
    if 0 < offset + fetch < n:
        assert s1["used_select"]
        assert min(n, offset + fetch) <= s1["candidates"] <= n
    return s1


def one_chunk(types, columns):
    n = len(columns[0][0]) if not isinstance(columns[0], Block) \
        else columns[0].n_rows
    return chunks_from_columns(types, columns, chunk_size=max(1, n))


def nulls(rng, n, frac):
    return (rng.random(n) < frac).astype(np.uint8)


# ---- golden ----------------------------------------------------------------

GOLD = [c for c in sr.load_golden() if c["device"]]


@pytest.mark.parametrize("null_last", [False, True])
@pytest.mark.parametrize("case", GOLD, ids=[c["name"] for c in GOLD])
def test_golden(hip, case, null_last):
    """Every reference test vector with numeric order columns, pushed chunk
    by chunk as the Java test pushes it; null_last either way changes
    nothing. A LimitExec case (no order column) orders by an added constant
    column: stability makes that LIMIT over arrival order."""
    types, chunks = sr.golden_chunks(case)
    order = sr.golden_order(case)
    strip = False
    if not order:
        types = types + [I32]
        chunks = [Chunk(c.blocks + [Block.of(I32, [7] * c.n_rows)])
                  for c in chunks]
        order, strip = [(len(types) - 1, True)], True
    exp = sr.golden_expected_rows(case)
    for select in (None, 0, 1):
        got, st, _ = run_device(hip, types, chunks, order, case["offset"],
                                case["fetch"], select, null_last=null_last)
        rows = sr.columns_rows(got)
        if strip:
            rows = [r[:-1] for r in rows]
        if case["compare"] == "multiset":
            assert sorted(map(repr, rows)) == sorted(map(repr, exp))
        else:
            assert rows == exp, (case["name"], select)


# ---- size edges --------------------------------------------------------------

BIG = 2 * 4096 * 256 + 1   # the grid-stride loop takes a 2nd and a 3rd trip


def _edge_data(n):
    rng = np.random.default_rng(1000 + n)
    k0 = rng.integers(-50, 50, n).astype(np.int64)
    k1 = rng.integers(0, 7, n).astype(np.int32)
    pay = np.arange(n, dtype=np.int64)
    types = [I64, I32, I64]
    cols = [(k0, nulls(rng, n, 0.1)), (k1, nulls(rng, n, 0.2)), (pay, None)]
    if n == 0:
        return types, [Chunk([Block(I64, values=k0), Block(I32, values=k1),
                              Block(I64, values=pay)])]
    return types, chunks_from_columns(types, cols, chunk_size=100)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 4095, 4097])
def test_size_edges(hip, n):
    types, chunks = _edge_data(n)
    order = [(0, False), (1, True)]
    cols = sr.concat_columns(chunks, types)
    perm = sr.sort_perm(cols, types, order)
    for fetch in sorted({0, 1, 10, n - 1, n, n + 5, -1} - {-2}):
        for offset in (0, 3, n + 2):
            for select in (0, 1):
                st, _ = check(hip, types, chunks, order, offset, fetch,
                              select, cols=cols, perm=perm)
                assert st["rows_consumed"] == n


def test_size_edge_grid_stride_trips(hip):
    """2*4096*256+1 rows, one pushed chunk, the default gate: small K runs
    the select, large K and the full sort do not."""
    n = BIG
    rng = np.random.default_rng(5)
    k0 = rng.integers(-(1 << 40), 1 << 40, n).astype(np.int64)
    pay = np.arange(n, dtype=np.int32)
    types = [I64, I32]
    chunks = one_chunk(types, [(k0, None), (pay, None)])
    order = [(0, True)]
    cols = sr.concat_columns(chunks, types)
    perm = sr.sort_perm(cols, types, order)
    for fetch in (0, 1, 10, n - 1, n, n + 5, -1):
        for offset in (0, 3, n + 2):
            st, _ = check(hip, types, chunks, order, offset, fetch,
                          cols=cols, perm=perm)
            k = offset + fetch
            if fetch > 0 and k <= n // 8:
                assert st["used_select"] and st["candidates"] < n // 8
            elif fetch != 0 and offset < n:
                assert not st["used_select"]


# ---- the select path -----------------------------------------------------------

def test_select_all_equal_first_column(hip):
    """Every row ties on column 0: the candidates are all rows and the other
    columns decide."""
    n = 70001
    rng = np.random.default_rng(11)
    types = [I64, I64, I32]
    chunks = one_chunk(types, [
        (np.full(n, 42, np.int64), None),
        (rng.integers(0, 1000, n).astype(np.int64), None),
        (np.arange(n, dtype=np.int32), None)])
    st = both_paths(hip, types, chunks, [(0, True), (1, False)], fetch=10)
    assert st["candidates"] == n
    assert st["select_passes"] == 6


def test_select_low_bits_only_runs_all_six_passes(hip):
    """Keys that differ only in their lowest 9 bits: no pass before the
    sixth can bring the candidates under the slack."""
    n = SELECT_SLACK + 5000
    rng = np.random.default_rng(12)
    k0 = ((0x1234567 << 9) + rng.integers(0, 512, n)).astype(np.int64)
    types = [I64, I32]
    chunks = one_chunk(types, [(k0, None), (np.arange(n, dtype=np.int32), None)])
    for asc in (True, False):
        st = both_paths(hip, types, chunks, [(0, asc)], fetch=10)
        assert st["select_passes"] == 6
        # the last bin holds the rows equal to the 10th key
        assert st["candidates"] < n // 100


def test_select_top_digit_exits_early(hip):
    n = SELECT_SLACK + 5000
    rng = np.random.default_rng(13)
    k0 = rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64)
    types = [I64, I32]
    chunks = one_chunk(types, [(k0, None), (np.arange(n, dtype=np.int32), None)])
    st = both_paths(hip, types, chunks, [(0, True)], fetch=10)
    assert 1 <= st["select_passes"] < 6
    assert st["candidates"] <= SELECT_SLACK


@pytest.mark.parametrize("dups", [1, 64, 1000])
def test_select_kth_value_duplicated_across_the_cut(hip, dups):
    n, k = 5000, 100
    rng = np.random.default_rng(14 + dups)
    below = max(0, k - 1 - dups // 2)   # the copies straddle rank K
    k0 = np.concatenate([rng.integers(0, 1000, below),
                         np.full(dups, 5000),                  # the K-th
                         rng.integers(9000, 1 << 40, n - below - dups)])
    k0 = k0[rng.permutation(n)].astype(np.int64)
    types = [I64, I32, I64]
    chunks = chunks_from_columns(types, [
        (k0, None), (rng.integers(0, 5, n).astype(np.int32), None),
        (np.arange(n, dtype=np.int64), None)], chunk_size=700)
    both_paths(hip, types, chunks, [(0, True)], fetch=k)
    both_paths(hip, types, chunks, [(0, True), (1, False)], fetch=k - 10,
               offset=10)


def test_select_int64_extremes(hip):
    n = 3000
    rng = np.random.default_rng(15)
    pool = np.array([I64_MIN, I64_MIN + 1, I64_MAX, I64_MAX - 1, -1, 0, 1,
                     -(1 << 62), 1 << 62, -12345], dtype=np.int64)
    k0 = pool[rng.integers(0, len(pool), n)]
    types = [I64, I32]
    chunks = chunks_from_columns(types, [
        (k0, nulls(rng, n, 0.05)), (np.arange(n, dtype=np.int32), None)],
        chunk_size=512)
    for asc in (True, False):
        both_paths(hip, types, chunks, [(0, asc)], fetch=400)
        both_paths(hip, types, chunks, [(0, asc)], fetch=7, offset=2)


def test_select_f64_specials(hip):
    n = 3000
    rng = np.random.default_rng(16)
    nan = lambda s, p: sr.pack_f64((s << 63) | (0x7ff << 52) | p)
    pool = np.array([0.0, -0.0, 5e-324, -5e-324, float("inf"), float("-inf"),
                     1.0, -1.0, 1e300, -1e300, nan(0, 1 << 51),
                     nan(1, 1 << 51), nan(0, 99), nan(1, (1 << 51) | 3)])
    k0 = pool[rng.integers(0, len(pool), n)]
    pay = pool[rng.integers(0, len(pool), n)]     # payload NaNs: bit-exact
    types = [F64, F64, I32]
    chunks = chunks_from_columns(types, [
        (k0, nulls(rng, n, 0.05)), (pay, None),
        (np.arange(n, dtype=np.int32), None)], chunk_size=512)
    for asc in (True, False):
        both_paths(hip, types, chunks, [(0, asc)], fetch=300)
        both_paths(hip, types, chunks, [(0, asc)], fetch=40, offset=5)
    check(hip, types, chunks, [(0, True)])


@pytest.mark.parametrize("asc", [True, False])
@pytest.mark.parametrize("n_null", [0, 5, 20, 50, 295, 300])
def test_select_null_count_around_k(hip, asc, n_null):
    """NULL count below, equal to and above K (and the mirror counts of
    non-NULL rows, which decide under DESC)."""
    n, k = 300, 20
    rng = np.random.default_rng(17 + n_null)
    nl = np.zeros(n, np.uint8)
    nl[rng.permutation(n)[:n_null]] = 1
    k0 = rng.integers(-100, 100, n).astype(np.int64)
    types = [I64, I32]
    chunks = chunks_from_columns(types, [
        (k0, nl), (np.arange(n, dtype=np.int32), None)], chunk_size=64)
    both_paths(hip, types, chunks, [(0, asc)], fetch=k)
    both_paths(hip, types, chunks, [(0, asc)], fetch=n - k)


def test_select_i32_first_column(hip):
    n = SELECT_SLACK + 3000
    rng = np.random.default_rng(18)
    k0 = rng.integers(-(1 << 31), (1 << 31) - 1, n).astype(np.int32)
    k0[:50] = [-(1 << 31), (1 << 31) - 1] * 25
    types = [I32, I64]
    chunks = one_chunk(types, [(k0, nulls(rng, n, 0.01)),
                               (np.arange(n, dtype=np.int64), None)])
    for asc in (True, False):   # K above the ~1% NULLs: values are needed
        st = both_paths(hip, types, chunks, [(0, asc)], fetch=2000)
        assert 1 <= st["select_passes"] <= 3
    # every key in one 11-bit bin of the first two digits: three passes
    k1 = (rng.integers(0, 1 << 10, n) + (5 << 10)).astype(np.int32)
    chunks = one_chunk(types, [(k1, None), (np.arange(n, dtype=np.int64), None)])
    st = both_paths(hip, types, chunks, [(0, True)], fetch=25)
    assert st["select_passes"] == 3


# ---- multi-column ---------------------------------------------------------------

@pytest.mark.parametrize("seed", range(20))
def test_multi_column_random(hip, seed):
    rng = np.random.default_rng(2000 + seed)
    n = 3000
    n_cols = 5
    types = [int(rng.choice([I64, I32, F64])) for _ in range(n_cols)]
    columns = []
    for ci, t in enumerate(types):
        card = 3 if ci < 2 else int(rng.choice([4, 50, 100000]))
        v = rng.integers(-card, card, n)
        if t == F64:
            v = v.astype(np.float64) / 2
        columns.append((v, nulls(rng, n, 0.15)))
    n_order = 1 + seed % 4
    ocols = [int(c) for c in rng.permutation(n_cols)[:n_order]]
    if seed % 2 == 0:
        ocols[0] = min(ocols[0], 1)      # a low-cardinality leading column
        ocols = list(dict.fromkeys(ocols))
    order = [(c, bool(rng.integers(0, 2))) for c in ocols]
    chunks = chunks_from_columns(types, columns, chunk_size=777)
    check(hip, types, chunks, order)
    both_paths(hip, types, chunks, order, fetch=int(rng.choice([1, 33, 500])),
               offset=int(rng.choice([0, 9])))


# ---- stability -------------------------------------------------------------------

def test_stability_on_heavily_tied_keys(hip):
    n = 20000
    rng = np.random.default_rng(31)
    types = [I32, F64, I64]
    chunks = chunks_from_columns(types, [
        (rng.integers(0, 4, n).astype(np.int32), nulls(rng, n, 0.2)),
        (rng.integers(0, 2, n).astype(np.float64), None),
        (np.arange(n, dtype=np.int64), None)], chunk_size=1000)
    for order in ([(0, True)], [(0, False), (1, True)], [(1, False)]):
        _, out = check(hip, types, chunks, order)
        # within a run of equal keys the arrival numbers ascend
        got = sr.concat_columns(out, types)
        arrival = got[2][0]
        same = np.ones(n - 1, bool)
        for c, _ in order:
            v, nl = got[c]
            same &= (nl[1:] == nl[:-1]) & ((v[1:] == v[:-1]) | (nl[1:] != 0))
        assert np.all(arrival[1:][same] > arrival[:-1][same])
        both_paths(hip, types, chunks, order, fetch=700, offset=3)


# ---- streaming compaction ------------------------------------------------------

@pytest.mark.parametrize("shape", ["random", "descending", "ascending"])
def test_streaming_compaction(hip, shape):
    n, k = 40 * 1000, 100
    rng = np.random.default_rng(41)
    if shape == "random":
        k0 = rng.integers(0, 5000, n)
    elif shape == "descending":     # every chunk displaces kept rows
        k0 = (n - np.arange(n)) // 3
    else:                           # no later chunk contributes
        k0 = np.arange(n) // 3
    types = [I64, I32, I64]
    chunks = chunks_from_columns(types, [
        (k0.astype(np.int64), nulls(rng, n, 0.01)),
        (rng.integers(0, 3, n).astype(np.int32), None),
        (np.arange(n, dtype=np.int64), None)], chunk_size=1000)
    order = [(0, True), (1, False)]
    for select in (0, 1):
        st, _ = check(hip, types, chunks, order, fetch=k - 5, offset=5,
                      select=select, compact_rows=2048)
        assert st["compactions"] >= 10
        assert st["rows_consumed"] == n
        assert st["rows_kept"] <= 2048 + 1000
        one, _ = check(hip, types, chunks, order, fetch=k - 5, offset=5,
                       select=select, compact_rows=1 << 30)
        assert one["compactions"] == 0 and one["rows_kept"] == n


# ---- payload ---------------------------------------------------------------------

def test_slice_and_decimal_payload(hip):
    n = 2500
    rng = np.random.default_rng(51)
    words = ["", "a", "bb", "polardb", "x" * 40, None]
    strs = [words[i] for i in rng.integers(0, len(words), n)]
    decs = [None if rng.random() < 0.1 else
            (int(rng.integers(-10 ** 12, 10 ** 12)), 2) for _ in range(n)]
    types = [I64, SLICE, DECIMAL, F64]
    columns = [(rng.integers(0, 40, n).astype(np.int64), nulls(rng, n, 0.1)),
               Block.of(SLICE, strs), Block.of(DECIMAL, decs),
               (rng.standard_normal(n), None)]
    chunks = chunks_from_columns(types, columns, chunk_size=600)
    check(hip, types, chunks, [(0, False)])
    both_paths(hip, types, chunks, [(0, True), (3, False)], fetch=123,
               offset=4)
    st, _ = check(hip, types, chunks, [(0, True)], fetch=50, select=1,
                  compact_rows=700)
    assert st["compactions"] >= 2


def test_null_free_column_has_no_nulls_buffer(hip):
    n = 500
    rng = np.random.default_rng(52)
    types = [I64, I32, F64]
    chunks = chunks_from_columns(types, [
        (rng.integers(0, 9, n).astype(np.int64), None),
        (rng.integers(0, 9, n).astype(np.int32), nulls(rng, n, 0.3)),
        (rng.standard_normal(n), None)], chunk_size=128)
    for fetch in (-1, 20):
        _, out = check(hip, types, chunks, [(1, True), (0, False)],
                       fetch=fetch)
        for ch in out:
            assert ch.blocks[0].nulls is None and ch.blocks[2].nulls is None
            assert ch.blocks[1].nulls is not None


def test_device_resident_input_chunks(hip):
    import torch
    n = 100000
    rng = np.random.default_rng(53)
    k0 = rng.integers(-1000, 1000, n).astype(np.int64)
    pay = rng.standard_normal(n)
    from galaxysql_amd.exchange import chunk_from_torch
    types = [I64, F64]
    order = [(0, False)]
    cols = [(k0, np.zeros(n, np.uint8)), (pay, np.zeros(n, np.uint8))]
    perm = sr.sort_perm(cols, types, order)
    for fetch, select in ((-1, None), (50, 1), (50, 0)):
        with select_mode(select):
            op = TopNExec(hip, order, types, fetch=fetch, device=0) \
                if fetch >= 0 else SortExec(hip, order, types, device=0)
        try:
            for lo in range(0, n, 30000):
                ts = [torch.from_numpy(a[lo:lo + 30000].copy()).cuda(0)
                      for a in (k0, pay)]
                ka = []
                op.consume_raw(C.byref(chunk_from_torch(hip, ts, types, ka)))
            op.build_consume()
            got = sr.concat_columns(op.result_chunks(), types)
        finally:
            op.close()
        assert_columns_equal(got, sr.gather_columns(
            cols, sr.limit(perm, 0, fetch)), types, order)


def test_out_chunk_rows_splits_into_ordered_batches(hip):
    n = 1000
    rng = np.random.default_rng(54)
    types = [I64, SLICE]
    chunks = chunks_from_columns(types, [
        (rng.integers(0, 300, n).astype(np.int64), None),
        Block.of(SLICE, [f"r{i}" for i in range(n)])], chunk_size=256)
    for fetch, want in ((-1, [300, 300, 300, 100]), (650, [300, 300, 50]),
                        (300, [300])):
        st, out = check(hip, types, chunks, [(0, True)], fetch=fetch,
                        out_chunk_rows=300)
        assert [c.n_rows for c in out] == want


# ---- validation --------------------------------------------------------------------

def _create(hip, types, order, **kw):
    return SortExec(hip, order, types, device=kw.pop("device", 0), **kw)


@pytest.mark.parametrize("what,kw", [
    ("no order column", dict(order=[])),
    ("nine order columns", dict(order=[(0, True)] * 9)),
    ("order col -1", dict(order=[(-1, True)])),
    ("order col past the schema", dict(order=[(4, True)])),
    ("SLICE order col", dict(order=[(2, True)])),
    ("DECIMAL order col", dict(order=[(3, True)])),
    ("offset < 0", dict(order=[(0, True)], offset=-1)),
    ("fetch < -1", dict(order=[(0, True)], fetch=-2)),
    ("device < 0", dict(order=[(0, True)], device=-1)),
])
def test_create_rejects(hip, what, kw):
    types = [I64, F64, SLICE, DECIMAL]
    with pytest.raises(RuntimeError) as e:
        _create(hip, types, **kw).close()
    msg = str(e.value)
    assert msg.startswith("gxop_sort_create: ") and \
        len(msg) > len("gxop_sort_create: "), what


def test_fetch_zero_passes_nothing(hip):
    types = [I64, I32]
    chunks = chunks_from_columns(types, [
        (np.arange(5000, dtype=np.int64), None),
        (np.arange(5000, dtype=np.int32), None)])
    for offset in (0, 7):
        got, st, out = run_device(hip, types, chunks, [(0, True)],
                                  offset=offset, fetch=0)
        assert out == []
        assert st["rows_consumed"] == 5000 and st["rows_kept"] == 0
        assert st["kernel_ms"] == 0.0 and st["compactions"] == 0


def test_next_before_build_is_an_error(hip):
    op = SortExec(hip, [(0, True)], [I64], device=0)
    try:
        op.consume_chunk(Chunk([Block.of(I64, [3, 1, 2])]))
        with pytest.raises(RuntimeError, match="before build"):
            op.result_chunks()
        op.build_consume()
        assert sr.columns_rows(sr.concat_columns(op.result_chunks(), [I64])) \
            == [(1,), (2,), (3,)]
        assert op.result_chunks() == []      # drained
    finally:
        op.close()


# ---- query chain ---------------------------------------------------------------------

def test_q3_order_limit(hip):
    """run_q3 leaves its groups on the device; q3_order_limit orders them
    there. Compared with the reference applied to the same emitted batches
    copied to the host: the values are identical, so equality is exact."""
    import torch
    from galaxysql_amd.queries import (run_q3, gen_q3_numpy, q3_order_limit,
                                       Q3_RESULT_TYPES)
    rng = np.random.default_rng(78)
    data = gen_q3_numpy(rng, n_cust_total=20000, n_orders_total=300000,
                        n_lineitem=1_200_000)
    t = [[torch.from_numpy(a).cuda(0) for a in cols] for cols in data]
    kept = []
    try:
        _, info = run_q3(hip, 0, t[0], t[1], t[2], to_host=False,
                         keep_results=kept)
        assert info["groups"] > 1000 and kept
        got10 = q3_order_limit(hip, 0, kept)
        got300 = q3_order_limit(hip, 0, kept, limit=300)
    finally:
        host = [hip.result_to_chunk(r) for r in kept]   # releases them
    order = [(3, False), (1, True)]
    exp = sr.columns_rows(sr.sort_ref(host, Q3_RESULT_TYPES, order, 0, 300))
    assert len(got10) == 10 and got10 == exp[:10]
    assert got300 == exp


def test_q18_order_limit(hip):
    import torch
    from galaxysql_amd.queries import (run_q18, gen_q18_numpy,
                                       q18_order_limit, Q18_RESULT_TYPES)
    rng = np.random.default_rng(79)
    data = gen_q18_numpy(rng, n_cust=5000, n_orders=100000,
                         having_frac=0.002)
    t = [[torch.from_numpy(a).cuda(0) for a in cols] for cols in data]
    kept = []
    try:
        n_final, _ = run_q18(hip, 0, t[0], t[1], t[2], keep_results=kept)
        assert n_final > 100 and len(kept) == 1
        got = q18_order_limit(hip, 0, kept)
    finally:
        host = [hip.result_to_chunk(r) for r in kept]
    exp = sr.columns_rows(sr.sort_ref(host, Q18_RESULT_TYPES,
                                      [(4, False), (2, True)], 0, 100))
    assert len(got) == 100 and got == exp
