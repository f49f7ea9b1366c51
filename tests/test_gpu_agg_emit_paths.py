"""Every aggregate func through every emission kernel of the HIP library:
the hash aggregation (slot-indexed, gid-indexed, LDS and gid-compaction
state), the group-join (one-kernel emission on the inline-bucket and CSR
tables, per-column emission behind a SLICE group column, the wide entries,
the COUNT(*)-as-matched path) and the frame window's whole-partition frame.

Reference: the CPU oracle. Inputs carry about 20 % NULLs and every case has a
group / position / partition whose inputs are all NULL. F64 inputs are
integer-valued with magnitude <= 1000, so every summation order gives the
same bits and the comparison is exact equality on the row multiset.

The group-join exposes no table choice; each of its cases is arranged so
that GroupJoinOp::do_build / next can take only the intended path (see the
case's comment), and the probe stats must agree with the oracle's counts."""
import functools

import numpy as np
import pytest

from galaxysql_amd import abi
from galaxysql_amd.chunk import (Block, F64, I32, I64, SLICE,
                                 chunks_from_columns, multiset, rows_of)
from galaxysql_amd.operators import (EquiJoinKey, HashAggExec,
                                     HashGroupJoinExec, run_agg, run_fwindow)

pytestmark = pytest.mark.gpu


def same(got, want):
    """exact: no rounding, -0.0 and +0.0 distinct"""
    assert multiset(got, f64_sign_zero=True) == \
        multiset(want, f64_sign_zero=True)


@pytest.fixture(scope="module")
def hip():
    return abi.load_hip()


# value columns, at these indices in every case: a I64, b I32, c F64
A, B, C_ = 1, 2, 3
AGGS13 = [(abi.COUNT_ROW, -1), (abi.COUNT_COL, B), (abi.SUM_I64, B),
          (abi.SUM_I64N, A), (abi.SUM_F64, C_), (abi.AVG_F64, C_),
          (abi.MIN_I64, A), (abi.MAX_I64, B), (abi.MIN_F64, C_),
          (abi.MAX_F64, C_), (abi.BIT_AND, A), (abi.BIT_OR, A),
          (abi.BIT_XOR, B)]
AGGS2 = [(abi.COUNT_ROW, -1), (abi.SUM_I64, B)]
TYPES = [I64, I64, I32, F64]


def value_columns(rng, n, dead):
    """a, b, c with 20 % NULLs each; rows under the mask `dead` all NULL"""
    a = rng.integers(-2 ** 40, 2 ** 40, n, dtype=np.int64)
    b = rng.integers(-2 ** 20, 2 ** 20, n).astype(np.int32)
    c = rng.integers(-1000, 1001, n).astype(np.float64)
    return [(v, ((rng.random(n) < 0.2) | dead).astype(np.uint8))
            for v in (a, b, c)]


# ---- 1. hash aggregation ----------------------------------------------------

@functools.lru_cache(maxsize=None)
def agg_data(n, global_agg=False):
    rng = np.random.default_rng(4100 + n)
    gk = rng.integers(0, 37, n, dtype=np.int64)
    gk[:37] = np.arange(37)
    cols = value_columns(rng, n, np.zeros(n, bool) if global_agg else gk == 36)
    if global_agg:   # the one group: column b all NULL
        cols[1] = (cols[1][0], np.ones(n, np.uint8))
    return [(gk, None)] + cols


@functools.lru_cache(maxsize=None)
def agg_want(n, aggs, global_agg=False, chunk_size=1000):
    chunks = chunks_from_columns(TYPES, agg_data(n, global_agg),
                                 chunk_size=chunk_size)
    gcols = [] if global_agg else [0]
    want = rows_of(run_agg(abi.load_oracle(), gcols, list(aggs), TYPES,
                           chunks, device=-1))
    assert len(want) == (1 if global_agg else 37)
    return chunks, want


def run_hip_agg(hip, gcols, aggs, chunks):
    op = HashAggExec(hip, gcols, aggs, TYPES, device=0)
    try:
        for ch in chunks:
            op.consume_chunk(ch)
        op.build_consume()
        return rows_of(op.result_chunks()), op.local_stats()
    finally:
        op.close()


def check_dead_group(want):
    dead = [r for r in want if r[0] == 36][0]
    # COUNT_ROW > 0, COUNT_COL = SUM_I64 = 0, the null-init funcs NULL,
    # BIT_AND all ones, BIT_OR / BIT_XOR 0
    assert dead[1] > 0 and dead[2:4] == (0, 0)
    assert all(v is None for v in dead[4:11])
    assert dead[11:] == (-1, 0, 0)


@pytest.mark.parametrize("case", ["narrow_slot", "wide_gid", "wide_lds"])
def test_agg_chunks(hip, monkeypatch, case):
    """4096 rows in chunks of 1000, 37 groups. narrow_slot: a 2-u64 record
    with group columns and no hint is slot-indexed and accumulates inside
    k_agg_insert; the 13 aggregates make a record wider than 4 u64, which is
    gid-indexed; with GX_AGG_LOCAL=1 its accumulate goes through LDS."""
    if case == "wide_lds":
        monkeypatch.setenv("GX_AGG_LOCAL", "1")
    else:
        monkeypatch.delenv("GX_AGG_LOCAL", raising=False)
    aggs = AGGS2 if case == "narrow_slot" else AGGS13
    chunks, want = agg_want(4096, tuple(aggs))
    if aggs is AGGS13:
        check_dead_group(want)
    got, st = run_hip_agg(hip, [0], aggs, chunks)
    same(got, want)
    assert st["local_rows"] == (4096 if case == "wide_lds" else 0)
    assert st["local_launches"] == (len(chunks) if case == "wide_lds" else 0)


def test_agg_gid_compaction(hip, monkeypatch):
    """one chunk of 2^18 rows: gids come from the compaction pass
    (k_agg_gid_*), the accumulate from the plain kernel"""
    monkeypatch.setenv("GX_AGG_LOCAL", "0")
    n = 1 << 18
    chunks, want = agg_want(n, tuple(AGGS13), chunk_size=n)
    assert len(chunks) == 1
    check_dead_group(want)
    got, st = run_hip_agg(hip, [0], AGGS13, chunks)
    same(got, want)
    assert st["local_rows"] == 0


def test_agg_global(hip, monkeypatch):
    monkeypatch.delenv("GX_AGG_LOCAL", raising=False)
    chunks, want = agg_want(4096, tuple(AGGS13), global_agg=True)
    assert want[0][1] == 0 and want[0][7] is None   # COUNT(b), MAX(b)
    got, _ = run_hip_agg(hip, [], AGGS13, chunks)
    same(got, want)
    # empty input: still one row, every null-init func NULL
    want = rows_of(run_agg(abi.load_oracle(), [], AGGS13, TYPES, [],
                           device=-1))
    assert len(want) == 1 and want[0][0] == 0 and want[0][3] is None
    got, _ = run_hip_agg(hip, [], AGGS13, [])
    same(got, want)


# ---- 2. group-join -----------------------------------------------------------

N_BUILD, N_PROBE = 300, 3000


@functools.lru_cache(maxsize=None)
def gj_data(null_build_key, with_slice):
    """consumed (key, pay I64, g2 I32[, name SLICE]); probe (key, a, b, c).
    Consumed keys come from 0..599, probe keys from 0..399: the keys above
    stay unmatched. Positions 5 and 6 share a key (two groups); every probe
    row of position 0's key has NULL inputs. Probe keys carry NULLs, which
    match only a NULL consumed key (null_build_key)."""
    rng = np.random.default_rng(4200)
    bk = rng.permutation(600)[:N_BUILD].astype(np.int64)
    bk[0] = 7
    bk[1:][bk[1:] == 7] = 599
    bk[6] = bk[5]
    assert (bk >= 400).sum() > 20
    bn = np.zeros(N_BUILD, np.uint8)
    if null_build_key:
        bn[11] = 1
    pay = rng.integers(0, 10 ** 6, N_BUILD, dtype=np.int64)
    g2 = rng.integers(0, 9, N_BUILD).astype(np.int32)
    g2n = (rng.random(N_BUILD) < 0.2).astype(np.uint8)
    btypes = [I64, I64, I32]
    bcols = [(bk, bn if null_build_key else None), (pay, None), (g2, g2n)]
    if with_slice:
        btypes.append(SLICE)
        bcols.append(Block.of(SLICE, [None if i % 13 == 3 else f"n{i % 41}"
                                      for i in range(N_BUILD)]))
    pk = rng.integers(0, 400, N_PROBE, dtype=np.int64)
    pk[:3] = 7
    pn = (rng.random(N_PROBE) < 0.05).astype(np.uint8)
    pn[:3] = 0
    vals = value_columns(rng, N_PROBE, pk == 7)
    build = chunks_from_columns(btypes, bcols)
    probe = chunks_from_columns(TYPES, [(pk, pn)] + vals)
    return btypes, build, probe


def run_gj(lib, device, join_type, btypes, build, probe, group_cols, aggs):
    op = HashGroupJoinExec(lib, join_type, [EquiJoinKey(0, 0, I64)], btypes,
                           TYPES, group_cols, aggs, device=device)
    try:
        for ch in build:
            op.consume_chunk(ch)
        op.build_consume()
        for ch in probe:
            op.probe_chunk(ch)
        rows = rows_of(op.result_chunks())
        return rows, (op.stats() if device >= 0 else None)
    finally:
        op.close()


# The oracle's group-join has no SUM_I64N (its accumulate leaves the state
# NULL), so the oracle runs the list without it. The HIP op runs all 13 with
# SUM_I64N over column b, next to COUNT_COL(b) and SUM_I64(b), and that one
# column is checked against SQL's definition: SUM_I64's value where any
# input was non-null, NULL where none was.
GJ_AGGS13 = [(abi.SUM_I64N, B) if f == abi.SUM_I64N else (f, c)
             for f, c in AGGS13]
I_SUMN = 3

AGGS_COUNT_FIRST = [(abi.COUNT_ROW, -1), (abi.MIN_I64, A), (abi.AVG_F64, C_),
                    (abi.MAX_F64, C_), (abi.BIT_AND, A)]

# name -> (NULL consumed key, SLICE group column, aggs, join types)
# The conditions of GroupJoinOp (gxhip_groupjoin.inc) each case relies on; if
# one of them changes, the case must be arranged anew:
#  inline: the ctor's `inline_ok` (one I64 key on both sides, `wide_ok` false:
#      more than 2 aggregates) and do_build_with's `inline_tab` (consumed key
#      column without has_nulls) -> inline-bucket table; next()'s
#      `fixed_width` (no SLICE group column) -> k_gj_emit_all
#  csr: has_nulls on the consumed key column makes `inline_tab` false, and
#      `wide_ok` is false -> the CSR table, k_gj_probe
#  slice: a SLICE group column makes next()'s `fixed_width` false ->
#      k_gather + k_agg_emit_col per column
#  wide: the ctor's `wide_ok` (<= 2 aggregates of COUNT / SUM_I64, one I64
#      key) and do_build_with's `wide` (key column without has_nulls)
#  count_first: `inline_tab`, INNER and a COUNT(*) set do_build_with's
#      `count_off` >= 0 -> no `used` bitmap in probe, compaction or emission
GJ_CASES = {
    "inline": (False, False, GJ_AGGS13, (abi.INNER, abi.LEFT)),
    "csr": (True, False, GJ_AGGS13, (abi.INNER, abi.LEFT)),
    "slice": (False, True, GJ_AGGS13, (abi.INNER, abi.LEFT)),
    "wide": (False, False, AGGS2, (abi.INNER, abi.LEFT)),
    "count_first": (False, False, AGGS_COUNT_FIRST, (abi.INNER,)),
}


@pytest.mark.parametrize("name,join_type", [
    (n, jt) for n, c in GJ_CASES.items() for jt in c[3]])
def test_groupjoin(hip, name, join_type):
    null_key, with_slice, aggs, _ = GJ_CASES[name]
    btypes, build, probe = gj_data(null_key, with_slice)
    gcols = [0, 2, 3] if with_slice else [0, 2]
    n_keys = len(gcols)
    all13 = aggs is GJ_AGGS13
    ora_aggs = [s for i, s in enumerate(aggs) if i != I_SUMN] if all13 \
        else aggs
    want, _ = run_gj(abi.load_oracle(), -1, join_type, btypes, build, probe,
                     gcols, ora_aggs)
    # position 0 (key 7) matched, by rows whose inputs are all NULL
    dead = [r for r in want if r[0] == 7]
    assert len(dead) == 1 and dead[0][n_keys] >= 3
    if all13:
        assert all(v is None for v in dead[0][n_keys + 3:n_keys + 9])
    if join_type == abi.LEFT:
        assert len(want) == N_BUILD
        assert sum(1 for r in want if r[0] is not None and r[0] >= 400) > 20
    else:
        assert 0 < len(want) < N_BUILD
    got, st = run_gj(hip, 0, join_type, btypes, build, probe, gcols, aggs)
    if all13:
        k = n_keys + I_SUMN
        for r in got:   # r[k - 2] = COUNT_COL(b), r[k - 1] = SUM_I64(b)
            assert r[k] == (r[k - 1] if r[k - 2] > 0 else None), r
        got = [r[:k] + r[k + 1:] for r in got]
    same(got, want)
    # COUNT(*) is the first aggregate of every list: over the INNER rows it
    # sums to the matches that the probe kernels counted
    inner = want if join_type == abi.INNER else run_gj(
        abi.load_oracle(), -1, abi.INNER, btypes, build, probe, gcols,
        ora_aggs)[0]
    assert st["matches"] == sum(r[n_keys] for r in inner)
    assert st["probe_launches"] == len(probe)
    assert st["probe_rows"] == N_PROBE


# ---- 3. frame window, whole partition ---------------------------------------

def test_fwindow_whole_partition(hip):
    n = 5000
    rng = np.random.default_rng(4300)
    part = np.sort(rng.integers(0, 50, n)).astype(np.int64)
    cols = [(part, None)] + value_columns(rng, n, part == 17)
    assert (part == 17).sum() > 1
    chunks = chunks_from_columns(TYPES, cols)
    frames = [(f, c, abi.FRAME_WHOLE_PARTITION) for f, c in AGGS13]
    want = rows_of(run_fwindow(abi.load_oracle(), [0], frames, TYPES, chunks,
                               device=-1))
    assert len(want) == n
    dead = [r for r in want if r[0] == 17][0]
    assert dead[4] > 1 and all(v is None for v in dead[7:14])
    got = rows_of(run_fwindow(hip, [0], frames, TYPES, chunks, device=0))
    same(got, want)
