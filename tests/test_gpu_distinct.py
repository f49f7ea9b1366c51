"""DISTINCT aggregates on the HIP path (gxop_agg_create with the
GX_AGG_*_DISTINCT funcs) against the two references of tests/distinct_ref.py:
the Python brute force and the two-level rewrite on the CPU oracle. Full
result-row multisets are compared (f64 rounded to 9 places, the suite's
convention; F64 inputs are small integers, so add order cannot move a sum).
Shapes are the smallest that reach each path: inline-gid small chunks,
the >= 262,144-row large-chunk mode, growth of both tables, one hot group,
the global aggregate."""
import numpy as np
import pytest

from galaxysql_amd import abi
from galaxysql_amd.chunk import (Block, Chunk, I64, I32, F64, SLICE,
                                 chunks_from_columns, multiset, rows_of)
from galaxysql_amd.operators import (EquiJoinKey, HashAggExec,
                                     HashGroupJoinExec,
                                     NonFrameOverWindowExec,
                                     OverWindowFramesExec, run_agg)

from . import distinct_ref as dr

pytestmark = pytest.mark.gpu

ALL5 = [abi.COUNT_DISTINCT, abi.SUM_I64_DISTINCT, abi.SUM_I64N_DISTINCT,
        abi.SUM_F64_DISTINCT, abi.AVG_F64_DISTINCT]


@pytest.fixture(scope="module")
def libs():
    import subprocess, os
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run(["make", "-C", os.path.join(repo, "oracle")], check=True,
                   capture_output=True)
    return abi.load_oracle(), abi.load_hip()


def ms(rows):
    return multiset(rows, f64_round=9)


def check(libs, group_cols, aggs, types, chunks, **kw):
    """HIP result rows == brute force == oracle rewrite, every row."""
    oracle, hip = libs
    got = rows_of(run_agg(hip, group_cols, aggs, types, chunks, device=0,
                          **kw))
    brute = dr.brute_agg(group_cols, aggs, chunks)
    rewrite = dr.rewrite_agg(oracle, group_cols, aggs, types, chunks)
    assert len(brute) == len(rewrite) and ms(brute) == ms(rewrite)
    assert len(got) == len(brute)
    assert ms(got) == ms(brute)
    return got


def nulls(rng, n, frac):
    return (rng.random(n) < frac).astype(np.uint8)


def test_golden_distinct_set(libs):
    gold = dr.load_golden()
    chunks = dr.golden_chunks(gold)
    got = check(libs, [0], [(abi.COUNT_DISTINCT, 1)], [I64, SLICE], chunks)
    assert multiset(got) == multiset(dr.golden_expected_rows(gold))


def _slice_col(rng, gk, n_vals, null_frac):
    """Strings of mixed length (some empty), per-group value ranges, NULLs."""
    n = len(gk)
    ids = gk * 3 + rng.integers(0, n_vals, n)
    isnull = rng.random(n) < null_frac
    return [None if isnull[i] else
            "" if ids[i] % 97 == 0 else
            "v" * int(ids[i] % 5) + str(int(ids[i])) for i in range(n)]


def test_slice_values_small_chunks(libs):
    """SLICE set across many chunks: every chunk is a DevStore append with
    an offset rebase, the set grows by occupancy, values include NULLs and
    empty strings; a plain agg rides along."""
    rng = np.random.default_rng(110)
    n = 6000
    gk = rng.integers(0, 150, n, dtype=np.int64)
    types = [I64, SLICE]
    chunks = chunks_from_columns(
        types, [(gk, nulls(rng, n, 0.05)),
                Block.of(SLICE, _slice_col(rng, gk, 12, 0.1))],
        chunk_size=997)
    assert len(chunks) == 7
    check(libs, [0], [(abi.COUNT_DISTINCT, 1), (abi.COUNT_ROW, -1)], types,
          chunks)


def test_slice_values_large_chunk_growth(libs):
    """SLICE set through a large-mode chunk that arrives AFTER a small one
    (nonzero rebase, owners from an earlier chunk) and overflows the set
    several times (pending-row reruns compare strings by drow), then small
    chunks that repeat earlier pairs."""
    rng = np.random.default_rng(111)
    n = 275_000
    gk = rng.integers(0, 20_000, n, dtype=np.int64)
    col = _slice_col(rng, gk, 40, 0.1)
    types = [I64, SLICE]
    cuts = [0, 3000, 268_000, 270_000, n]
    chunks = [Chunk([Block(I64, values=gk[a:b]), Block.of(SLICE, col[a:b])])
              for a, b in zip(cuts, cuts[1:])]
    assert chunks[1].n_rows >= 1 << 18
    check(libs, [0], [(abi.COUNT_DISTINCT, 1)], types, chunks,
          expected_groups=16)


def test_all_funcs_with_plain_aggs(libs):
    rng = np.random.default_rng(101)
    n = 50_000
    gk = rng.integers(0, 3000, n, dtype=np.int64)
    types = [I64, I64, F64, I32]
    chunks = chunks_from_columns(types, [
        (gk, None),
        (gk * 31 + rng.integers(0, 20, n), nulls(rng, n, 0.1)),
        ((gk % 7 + rng.integers(0, 20, n)).astype(np.float64), None),
        (rng.integers(-10, 10, n, dtype=np.int32), nulls(rng, n, 0.05))],
        chunk_size=997)
    aggs = [(abi.COUNT_ROW, -1), (abi.SUM_I64, 1), (abi.MIN_I64, 1),
            (abi.COUNT_DISTINCT, 1), (abi.SUM_I64_DISTINCT, 1),
            (abi.SUM_I64N_DISTINCT, 1), (abi.SUM_F64_DISTINCT, 1),
            (abi.COUNT_DISTINCT, 2), (abi.SUM_F64_DISTINCT, 2),
            (abi.AVG_F64_DISTINCT, 2),
            (abi.COUNT_DISTINCT, 3), (abi.SUM_I64_DISTINCT, 3),
            (abi.SUM_I64N_DISTINCT, 3), (abi.AVG_F64_DISTINCT, 3)]
    check(libs, [0], aggs, types, chunks)


def test_count_distinct_only(libs):
    """Record stride 1: a plain op of this width takes the slot-records
    path, which a distinct op must not."""
    rng = np.random.default_rng(102)
    n = 20_000
    gk = rng.integers(0, 500, n, dtype=np.int64)
    chunks = chunks_from_columns(
        [I64, I64], [(gk, None), (rng.integers(0, 15, n), nulls(rng, n, 0.1))],
        chunk_size=997)
    check(libs, [0], [(abi.COUNT_DISTINCT, 1)], [I64, I64], chunks)


def test_large_chunk_mode(libs):
    """One chunk >= 262,144 rows: gids are pending during the group insert
    and both tables start at their minimum and grow by overflow retry."""
    rng = np.random.default_rng(103)
    n = 300_000
    gk = rng.integers(0, 40_000, n, dtype=np.int64)
    types = [I64, I64, F64]
    chunks = chunks_from_columns(types, [
        (gk, None), (rng.integers(0, 6, n) - gk, nulls(rng, n, 0.05)),
        (rng.integers(0, 4, n).astype(np.float64), None)], chunk_size=n)
    assert len(chunks) == 1
    check(libs, [0], [(abi.COUNT_ROW, -1), (abi.COUNT_DISTINCT, 1),
                      (abi.SUM_I64_DISTINCT, 1), (abi.AVG_F64_DISTINCT, 2)],
          types, chunks)


def test_chunking_does_not_change_result(libs):
    rng = np.random.default_rng(104)
    n = 60_000
    gk = rng.integers(0, 2000, n, dtype=np.int64)
    cols = [(gk, None), (rng.integers(0, 25, n), nulls(rng, n, 0.1))]
    types = [I64, I64]
    aggs = [(abi.COUNT_DISTINCT, 1), (abi.SUM_I64N_DISTINCT, 1)]
    one = chunks_from_columns(types, cols, chunk_size=n)
    cuts = [0, 1, 998, 5000, 5001, 31_000, 59_999, n]
    uneven = []
    for a, b in zip(cuts, cuts[1:]):
        uneven += chunks_from_columns(
            types, [(v[a:b], None if m is None else m[a:b]) for v, m in cols],
            chunk_size=n)
    assert len(one) == 1 and len(uneven) == 7
    g1 = check(libs, [0], aggs, types, one)
    g7 = check(libs, [0], aggs, types, uneven)
    assert multiset(g1) == multiset(g7)


def test_both_tables_grow_mid_stream(libs):
    """expected_groups=16 with ~200k distinct (group, value) pairs: a
    large-mode chunk forces overflow growth with pending-row reruns, the
    small chunks after it grow by occupancy."""
    rng = np.random.default_rng(105)
    n = 300_000
    gk = rng.integers(0, 30_000, n, dtype=np.int64)
    vals = rng.integers(0, 1 << 40, n)
    k = n // 3                             # a third of the rows are repeats
    vals[-k:] = vals[:k]
    gk[-k:] = gk[:k]
    perm = rng.permutation(n)
    gk, vals = gk[perm], vals[perm]
    types = [I64, I64]
    big = 265_000
    chunks = chunks_from_columns(types, [(gk[:big], None), (vals[:big], None)],
                                 chunk_size=big)
    chunks += chunks_from_columns(types, [(gk[big:], None), (vals[big:], None)],
                                  chunk_size=5000)
    check(libs, [0], [(abi.COUNT_DISTINCT, 1), (abi.SUM_I64_DISTINCT, 1)],
          types, chunks, expected_groups=16)


def test_hot_pair(libs):
    """One group, three values, 100k rows: every lane fights for 3 slots."""
    rng = np.random.default_rng(106)
    n = 100_000
    types = [I64, I64]
    chunks = chunks_from_columns(
        types, [(np.full(n, 7, np.int64), None),
                (rng.integers(0, 3, n) * 1000, None)], chunk_size=n)
    got = check(libs, [0], [(abi.COUNT_DISTINCT, 1),
                            (abi.SUM_I64_DISTINCT, 1), (abi.COUNT_ROW, -1)],
                types, chunks)
    assert got == [(7, 3, 3000, n)]


def test_global_aggregate(libs):
    rng = np.random.default_rng(107)
    n = 30_000
    types = [I64, F64]
    aggs = [(f, 0) for f in ALL5] + [(abi.COUNT_DISTINCT, 1),
                                     (abi.AVG_F64_DISTINCT, 1)]
    chunks = chunks_from_columns(types, [
        (rng.integers(-50, 50, n), nulls(rng, n, 0.1)),
        (rng.integers(0, 9, n).astype(np.float64), nulls(rng, n, 0.1))],
        chunk_size=997)
    check(libs, [], aggs, types, chunks)


def test_global_aggregate_all_null(libs):
    n = 3000
    types = [I64, F64]
    aggs = [(f, 0) for f in ALL5] + [(abi.SUM_F64_DISTINCT, 1)]
    chunks = chunks_from_columns(types, [
        (np.zeros(n, np.int64), np.ones(n, np.uint8)),
        (np.zeros(n), np.ones(n, np.uint8))], chunk_size=997)
    got = check(libs, [], aggs, types, chunks)
    assert got == [(0, 0, None, None, None, None)]


def test_global_aggregate_empty_input(libs):
    aggs = [(f, 0) for f in ALL5]
    got = check(libs, [], aggs, [I64], [])
    assert got == [(0, 0, None, None, None)]


def test_null_group_keys(libs):
    rng = np.random.default_rng(108)
    n = 12_000
    types = [I64, I64]
    chunks = chunks_from_columns(types, [
        (rng.integers(0, 40, n), nulls(rng, n, 0.2)),
        (rng.integers(0, 30, n), nulls(rng, n, 0.1))], chunk_size=997)
    got = check(libs, [0], [(abi.COUNT_DISTINCT, 1),
                            (abi.SUM_I64_DISTINCT, 1)], types, chunks)
    assert sum(1 for r in got if r[0] is None) == 1


def test_multi_key_grouping(libs):
    """(I32, I64) keys take the packed key path, independent of the set."""
    rng = np.random.default_rng(109)
    n = 40_000
    types = [I32, I64, I64]
    chunks = chunks_from_columns(types, [
        (rng.integers(0, 60, n, dtype=np.int32), nulls(rng, n, 0.05)),
        (rng.integers(0, 50, n), None),
        (rng.integers(0, 12, n), nulls(rng, n, 0.1))], chunk_size=3000)
    check(libs, [0, 1], [(abi.COUNT_DISTINCT, 2), (abi.SUM_I64N_DISTINCT, 2),
                         (abi.COUNT_ROW, -1)], types, chunks)


# ---- rejections: assert on the text (create on the HIP library can fail for
# other reasons too) ----

def _err(fn):
    with pytest.raises(RuntimeError) as e:
        fn()
    return str(e.value)


@pytest.mark.parametrize("func", ALL5)
def test_other_ops_reject_distinct(libs, func):
    _, hip = libs
    msg = _err(lambda: HashGroupJoinExec(
        hip, abi.INNER, [EquiJoinKey(0, 0, I64)], [I64], [I64, I64],
        group_cols=[0], aggs=[(func, 1)], device=0))
    assert "DISTINCT" in msg and "group-join" in msg
    msg = _err(lambda: NonFrameOverWindowExec(
        hip, [0], [(func, 1)], [I64, I64], device=0))
    assert "DISTINCT" in msg and "window" in msg
    msg = _err(lambda: OverWindowFramesExec(
        hip, [0], [(func, 1, abi.FRAME_WHOLE_PARTITION, 0, 0)], [I64, I64],
        device=0))
    assert "DISTINCT" in msg and "frame-window" in msg


def test_create_rejects_bad_input(libs):
    _, hip = libs
    msg = _err(lambda: HashAggExec(hip, [0], [(abi.SUM_I64_DISTINCT, 1)],
                                   [I64, SLICE], device=0))
    assert "DISTINCT" in msg and "input type" in msg
    for func in ALL5[1:]:
        assert "input type" in _err(lambda: HashAggExec(
            hip, [0], [(func, 1)], [I64, SLICE], device=0))
    # the integer sums take I64/I32 only: the base funcs would read a
    # double's bits as an integer
    for func in (abi.SUM_I64_DISTINCT, abi.SUM_I64N_DISTINCT):
        msg = _err(lambda: HashAggExec(hip, [0], [(func, 1)], [I64, F64],
                                       device=0))
        assert "DISTINCT" in msg and "input type" in msg
    for col in (-1, 2):
        msg = _err(lambda: HashAggExec(hip, [0], [(abi.COUNT_DISTINCT, col)],
                                       [I64, I64], device=0))
        assert "DISTINCT" in msg and "out of range" in msg
