"""Transposed accumulate of the group-join probe-scan, and the `used` bitmap
that an INNER op with COUNT(*) no longer keeps.

For a record of up to 4 u64 whose aggregates are all additive the fused
kernel's flush turns each 64 staged matches round: W = the power of two >=
the record's stride, W passes, lanes L..L+W-1 of one atomic instruction
cover the slots of one record. The cases are the shapes at which that can go
wrong: flush sizes around W, 16, 64 and the 384-pair stage, every stride,
many lanes of one instruction on one word or one line, NULL inputs, the
shapes that must keep the per-lane loop, and ops with and without the
bitmap. As in test_gpu_groupjoin_probe_scan (whose generators and run_case
these reuse) every case compares the fused call, the composed scan-then-probe
path and, where cheap, the CPU oracle as multisets of rows, over dyadic f64
inputs, so integers, counts and f64 sums compare with ==; n_matched is
checked against numpy.

A group-join of at most two COUNT/SUM_I64 aggregates keeps its state in the
CSR wide entries, so the stride-1 and SUM_I64 + COUNT_ROW cases run the
composed path on both sides; SUM_F64 alone and SUM_I64N alone are the
stride-2 records that reach the fused kernel.
"""
import ctypes as C

import numpy as np
import pytest

from galaxysql_amd import abi
from galaxysql_amd.chunk import rows_of
from galaxysql_amd.operators import HashGroupJoinExec, ScanExec

from .test_gpu_groupjoin_probe_scan import (
    ALL, HALF, BUILD_TYPES, KEYS, OUT_TYPES, PROJS, Q3_AGGS, RAW_TYPES,
    dev_chunk, gen_build, gen_raw, host_chunk, pred_mask, rows, run_case,
    take_rows)

pytestmark = pytest.mark.gpu

# records by stride; oracle=False where the set holds a SUM_I64N (the
# oracle's group-join has no case for it)
S2_F64 = [(abi.SUM_F64, 1)]
S2_I64N = [(abi.SUM_I64N, 4)]
S3 = [(abi.SUM_F64, 1), (abi.COUNT_ROW, -1)]
S4_AVG = [(abi.AVG_F64, 5), (abi.SUM_I64N, 2)]

N_SIX, N_SINGLE = 20, 110


def edge_build(rng):
    """20 keys consumed six times each (runs past the 4 inline slots) and
    110 keys consumed once, shuffled."""
    k6 = np.arange(N_SIX, dtype=np.int64) * 3 + 1
    k1 = (N_SIX + np.arange(N_SINGLE, dtype=np.int64)) * 3 + 1
    keys = np.concatenate([np.repeat(k6, 6), k1])
    rng.shuffle(keys)
    n = len(keys)
    return [(keys, None), (rng.integers(0, 1000, n).astype(np.int32), None),
            (np.arange(n, dtype=np.int64), None)]


def edge_raw(rng, matches):
    """128 rows, the tile of ONE wave, of which exactly `matches` (row,
    position) pairs match: every pair passes through that wave's stage."""
    six, single = (0, matches) if matches <= N_SINGLE else (60, matches - 360)
    assert 0 <= single <= 128 - six
    raw = gen_raw(rng, 128, 1, match="none")
    key = raw[0][0]
    key[:] = 2                                      # matches nothing
    key[:six] = rng.integers(0, N_SIX, six) * 3 + 1
    key[six:six + single] = \
        (N_SIX + rng.integers(0, N_SINGLE, single)) * 3 + 1
    rng.shuffle(key)
    return raw


@pytest.mark.parametrize("aggs", [Q3_AGGS, S3, S2_F64, S2_I64N],
                         ids=["stride4", "stride3", "stride2f", "stride2i"])
@pytest.mark.parametrize("matches", [1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65,
                                     383, 384, 385])
def test_pass_edges(matches, aggs):
    rng = np.random.default_rng(matches)
    _, _, _, _, kept, matched = run_case(
        edge_raw(rng, matches), edge_build(rng), ALL, aggs=aggs,
        oracle=aggs is not S2_I64N)
    assert kept == 128 and matched == matches


@pytest.mark.parametrize("aggs,oracle", [
    ([(abi.COUNT_ROW, -1)], True),                      # stride 1 (wide mode)
    ([(abi.SUM_I64, 2), (abi.COUNT_ROW, -1)], True),    # stride 2 (wide mode)
    (S2_F64, True), (S2_I64N, False),                   # stride 2
    (S3, True),                      # stride 3: records straddle 64-B lines
    (Q3_AGGS, True), (S4_AVG, False),                   # stride 4
], ids=["s1", "s2wide", "s2f", "s2i", "s3", "s4q3", "s4avg"])
def test_every_fast_path_stride(aggs, oracle):
    rng = np.random.default_rng(31)
    got, *_ = run_case(gen_raw(rng, 3000, 70, match="all", null_cols=(2, 4)),
                       gen_build(rng, 70), HALF, aggs=aggs, oracle=oracle)
    assert sum(c.n_rows for c in got) == 70


@pytest.mark.parametrize("aggs", [Q3_AGGS, S3, S2_F64],
                         ids=["stride4", "stride3", "stride2"])
def test_all_matches_on_one_record(aggs):
    """Every lane of every atomic instruction on one record's words."""
    rng = np.random.default_rng(32)
    raw = gen_raw(rng, 3000, 10, match="one")
    got, _, _, _, _, matched = run_case(raw, gen_build(rng, 10), ALL,
                                        aggs=aggs)
    (r,) = rows_of(got)
    price, disc = raw[2][0], raw[3][0]
    assert matched == 3000 and r[3] == float((price * (1.0 - disc)).sum())


def test_all_matches_on_one_key_consumed_six_times():
    """match="one" against a key consumed 6x: each probe row is staged six
    times, for six records."""
    rng = np.random.default_rng(33)
    got, _, _, _, _, matched = run_case(gen_raw(rng, 2000, 10, match="one"),
                                        gen_build(rng, 10, dup=6), ALL)
    out = rows_of(got)
    assert matched == 6 * 2000 and len(out) == 6
    assert len({r[3:] for r in out}) == 1 and out[0][5] == 2000


@pytest.mark.parametrize("aggs", [Q3_AGGS, S3], ids=["stride4", "stride3"])
def test_all_matches_on_two_adjacent_records(aggs):
    """Positions 0 and 1: stride 4 puts both records in one 64-B line."""
    rng = np.random.default_rng(34)
    build = gen_build(rng, 10)
    build[0] = (np.arange(10, dtype=np.int64) * 3 + 1, None)   # unshuffled
    raw = gen_raw(rng, 3000, 10, match="one")
    raw[0][0][:] = rng.integers(0, 2, 3000) * 3 + 1            # keys 1 and 4
    got, _, _, _, _, matched = run_case(raw, build, ALL, aggs=aggs)
    out = sorted(rows_of(got))
    assert matched == 3000 and [r[2] for r in out] == [0, 1]
    assert out[0][-1] + out[1][-1] == 3000


@pytest.mark.parametrize("aggs,oracle", [
    (S3, True), ([(abi.AVG_F64, 5), (abi.COUNT_ROW, -1)], True),
    ([(abi.SUM_I64N, 4), (abi.COUNT_ROW, -1)], False),
    ([(abi.SUM_F64, 1), (abi.COUNT_COL, 2), (abi.COUNT_ROW, -1)], True),
], ids=["sum_f64", "avg_f64", "sum_i64n", "count_col"])
def test_null_inputs_and_an_all_null_group(aggs, oracle):
    """30 % NULL inputs, every input of key 1 NULL: its SUM/AVG is NULL and
    COUNT(*) still counts its rows."""
    rng = np.random.default_rng(35)
    raw = gen_raw(rng, 3000, 12, match="all", null_cols=(2, 4))
    mine = raw[0][0] == 1
    raw[2][1][mine] = 1
    raw[4][1][mine] = 1
    got, *_ = run_case(raw, gen_build(rng, 12), ALL, aggs=aggs, oracle=oracle)
    (r,) = [x for x in rows_of(got) if x[0] == 1]
    assert r[3] is None and r[-1] == int(mine.sum()) > 0
    if len(aggs) == 3:
        assert r[4] == 0                                   # COUNT_COL
    assert all(x[3] is not None for x in rows_of(got) if x[0] != 1)


@pytest.mark.parametrize("aggs", [
    [(abi.MIN_I64, 3), (abi.COUNT_ROW, -1)],               # 3 u64, not additive
    [(abi.MIN_F64, 1), (abi.MAX_I64, 4), (abi.COUNT_ROW, -1)],
    [(abi.BIT_OR, 2), (abi.BIT_XOR, 4), (abi.BIT_AND, 3), (abi.COUNT_ROW, -1)],
    [(abi.BIT_OR, 2), (abi.SUM_F64, 1)],                   # no COUNT(*)
    Q3_AGGS + [(abi.AVG_F64, 5)],                          # 6 u64
], ids=["min", "minmax", "bit", "bit_nocount", "wide"])
def test_fallback_shapes_keep_their_answers(aggs):
    rng = np.random.default_rng(36)
    got, *_ = run_case(gen_raw(rng, 3000, 40, match="all", null_cols=(1, 3)),
                       gen_build(rng, 40), HALF, aggs=aggs)
    assert sum(c.n_rows for c in got) == 40


def n_matched_positions(raw, build, preds):
    live = set(raw[0][0][pred_mask(raw, preds)].tolist())
    return sum(int(k) in live for k in build[0][0])


@pytest.mark.parametrize("what", ["count_row", "no_count_row", "left"])
def test_used_elision(what):
    """The same data through an INNER op with COUNT(*) (no bitmap: matched =
    count != 0), an INNER op without it and a LEFT op (bitmap kept; its
    unmatched groups still get count_row_null_row's 1)."""
    rng = np.random.default_rng(37)
    raw, build = gen_raw(rng, 2500, 300), gen_build(rng, 300)
    want = n_matched_positions(raw, build, HALF)
    assert 0 < want < 300
    aggs = {"count_row": Q3_AGGS, "left": Q3_AGGS,
            "no_count_row": [(abi.SUM_F64, 1), (abi.COUNT_COL, 2)]}[what]
    got, *_ = run_case(raw, build, HALF, aggs=aggs,
                       join_type=abi.LEFT if what == "left" else abi.INNER)
    out = rows_of(got)
    if what == "left":
        assert len(out) == 300
        unmatched = [r for r in out if r[3] is None]
        assert len(unmatched) == 300 - want
        assert all(r[4] == 0 and r[5] == 1 for r in unmatched)
    else:
        assert len(out) == want


@pytest.mark.parametrize("aggs", [Q3_AGGS, [(abi.SUM_F64, 1),
                                            (abi.COUNT_COL, 2)]],
                         ids=["elided", "bitmap"])
def test_mixed_probe_calls_on_one_op(aggs):
    """One fused call and one plain gxop_groupjoin_probe call on the same
    op, then next: both kernels must agree on where "matched" lives. The
    plain call's chunk reaches positions the fused call did not."""
    rng = np.random.default_rng(38)
    hip, orc = abi.load_hip(), abi.load_oracle()
    build_cols = gen_build(rng, 200)
    build = host_chunk(build_cols, BUILD_TYPES)
    raw1, raw2 = gen_raw(rng, 1500, 200), gen_raw(rng, 1500, 200)

    def make(lib, device):
        g = HashGroupJoinExec(lib, abi.INNER, KEYS, BUILD_TYPES, OUT_TYPES,
                              [0, 1, 2], aggs, device=device)
        g.consume_chunk(build)
        g.build_consume()
        return g

    go = make(orc, -1)
    so = ScanExec(orc, [], PROJS, RAW_TYPES, device=-1)
    try:
        for raw in (raw1, raw2):
            m = pred_mask(raw, HALF)
            go.probe_chunk(so.consume_chunk(
                host_chunk(take_rows(raw, RAW_TYPES, m), RAW_TYPES)))
        ref = go.result_chunks()
    finally:
        go.close()
        so.close()

    ga, gb = make(hip, 0), make(hip, 0)
    s = ScanExec(hip, HALF, PROJS, RAW_TYPES, device=0)
    try:
        ka = []
        c1 = dev_chunk(hip, raw1, RAW_TYPES, ka)
        c2 = dev_chunk(hip, raw2, RAW_TYPES, ka)

        def plain(g, c):
            t = s.consume_raw(C.byref(c))
            hip.check(hip.lib.gxop_groupjoin_probe(
                g._op, C.byref(t.contents.chunk)), "groupjoin_probe")
            hip.lib.gxop_result_release(t)

        ga.probe_scan(s, C.byref(c1))       # fused, then plain
        plain(ga, c2)
        plain(gb, c1)                       # plain, then fused
        gb.probe_scan(s, C.byref(c2))
        got_a, got_b = ga.result_chunks(), gb.result_chunks()
        matches = ga.stats()["matches"], gb.stats()["matches"]
    finally:
        ga.close()
        gb.close()
        s.close()
    both = [(np.concatenate([raw1[c][0], raw2[c][0]]), None) for c in (0, 1)]
    want = n_matched_positions(both, build_cols, [(1, abi.GT, 49)])
    alone = n_matched_positions(raw1, build_cols, HALF)
    print(f"positions matched by both chunks {want}, by the first {alone}")
    assert alone < want == sum(c.n_rows for c in got_a)
    assert matches[0] == matches[1]
    assert rows(got_a) == rows(ref) and rows(got_b) == rows(ref)


def test_arbitrary_doubles_within_bound():
    """Inexact sums through the transposed adds: any two summation orders of
    m positive terms differ by at most (m - 1) * 2^-52 relative."""
    rng = np.random.default_rng(39)
    raw = gen_raw(rng, 6000, 40, match="all", dyadic=False)
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
