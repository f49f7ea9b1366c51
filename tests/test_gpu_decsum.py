"""Exact DECIMAL SUM / AVG on the HIP hash aggregation (GX_AGG_SUM_DEC /
GX_AGG_AVG_DEC, 128-bit state) against tests/decsum_ref.py: Python integer
sums, compared exactly as multisets of rows with DECIMAL cells decoded to
(scaled value, scale). Shapes are the smallest that reach each path: the
slot-fused insert and the gid-indexed accumulate, small inline-gid chunks
and the >= 262,144-row large-chunk mode, table growth with the failed-row
rerun, one hot group, the global aggregate, DECIMAL-record input with its
fences."""
import functools

import numpy as np
import pytest

from galaxysql_amd import abi
from galaxysql_amd.chunk import (Block, Chunk, DECIMAL, F64, I32, I64, SLICE,
                                 chunks_from_columns, dec40_encode_wide)
from galaxysql_amd.exchange import final_agg_specs
from galaxysql_amd.operators import (EquiJoinKey, HashAggExec,
                                     HashGroupJoinExec,
                                     NonFrameOverWindowExec,
                                     OverWindowFramesExec, run_agg)

from . import decsum_ref as ref

pytestmark = pytest.mark.gpu

I64_MAX, I64_MIN = 2 ** 63 - 1, -2 ** 63
PALETTE = np.array([I64_MAX, I64_MIN, 2 ** 62, -2 ** 62, 7, -3, 0, 1],
                   dtype=np.int64)


@pytest.fixture(scope="module")
def hip():
    return abi.load_hip()


def run(hip, group_cols, aggs, types, chunks, **kw):
    return ref.result_rows(run_agg(hip, group_cols, aggs, types, chunks,
                                   device=0, **kw))


def pyvals(vals, nulls):
    return [None if (nulls is not None and nulls[i]) else int(vals[i])
            for i in range(len(vals))]


def wrap64(v):
    return (v + 2 ** 63) % 2 ** 64 - 2 ** 63


@functools.lru_cache(maxsize=None)
def carry_data():
    """3,000 groups x ~17 rows of extreme and small values; groups >= 2,900
    are all NULL; every group mixes signs, so its running sum crosses zero
    and wraps the low word in both directions."""
    rng = np.random.default_rng(2801)
    n = 51_000
    gk = rng.integers(0, 3000, n, dtype=np.int64)
    vals = PALETTE[rng.integers(0, len(PALETTE), n)]
    nulls = ((rng.random(n) < 0.1) | (gk >= 2900)).astype(np.uint8)
    keys = [(int(k),) for k in gk]
    pv = pyvals(vals, nulls)
    chunks = chunks_from_columns([I64, I64], [(gk, None), (vals, nulls)],
                                 chunk_size=997)
    return keys, pv, chunks, ref.ref_sum(keys, pv, 0)


def test_carry_slot_fused(hip):
    """SUM_DEC alone: a 3-slot record, accumulated inside k_agg_insert."""
    keys, pv, chunks, want = carry_data()
    assert any(c is None for c in want.values())
    assert any(c is not None and abs(c[0]) >= 2 ** 64 for c in want.values())
    got = run(hip, [0], [(abi.sum_dec(0), 1)], [I64, I64], chunks)
    ref.same(got, ref.expected_rows(want))


def test_carry_gid_path(hip):
    """With three more aggregates the record is 8 slots: gid-indexed state
    and the separate accumulate pass."""
    keys, pv, chunks, want = carry_data()
    cnt, s64, mn = {}, {}, {}
    for k, v in zip(keys, pv):
        cnt[k] = cnt.get(k, 0) + 1
        s64.setdefault(k, None)
        mn.setdefault(k, None)
        if v is not None:
            s64[k] = wrap64((s64[k] or 0) + v)
            mn[k] = v if mn[k] is None else min(mn[k], v)
    aggs = [(abi.COUNT_ROW, -1), (abi.SUM_I64N, 1), (abi.MIN_I64, 1),
            (abi.sum_dec(0), 1)]
    got = run(hip, [0], aggs, [I64, I64], chunks)
    ref.same(got, ref.expected_rows(cnt, s64, mn, want))


def test_slot_stride_2_equals_default(hip, monkeypatch):
    """GX_AGG_SLOT_STRIDE=2 sends the 3-slot record down the gid path."""
    keys, pv, chunks, want = carry_data()
    default = run(hip, [0], [(abi.sum_dec(0), 1)], [I64, I64], chunks)
    monkeypatch.setenv("GX_AGG_SLOT_STRIDE", "2")
    narrow = run(hip, [0], [(abi.sum_dec(0), 1)], [I64, I64], chunks)
    ref.same(narrow, default)
    ref.same(narrow, ref.expected_rows(want))


def test_one_hot_group(hip):
    """300,000 rows into one group in one large-mode chunk: the carry race
    under maximal contention. INT64_MAX and INT64_MIN+1 in random order
    cancel; a trailing run of INT64_MAX takes the sum past 2^64."""
    rng = np.random.default_rng(2802)
    half, tail = 149_500, 1000
    body = np.concatenate([np.full(half, I64_MAX, dtype=np.int64),
                           np.full(half, I64_MIN + 1, dtype=np.int64)])
    rng.shuffle(body)
    vals = np.concatenate([body, np.full(tail, I64_MAX, dtype=np.int64)])
    n = len(vals)
    assert n == 300_000 and n >= 1 << 18
    total = tail * I64_MAX
    assert total > 2 ** 64
    chunk = Chunk([Block(I64, values=np.zeros(n, dtype=np.int64)),
                   Block(I64, values=vals)])
    got = run(hip, [0], [(abi.sum_dec(0), 1)], [I64, I64], [chunk])
    ref.same(got, [(0, (total, 0))])
    got = run(hip, [0], [(abi.COUNT_ROW, -1), (abi.avg_dec(0), 1),
                         (abi.sum_dec(0), 1)], [I64, I64], [chunk])
    ref.same(got, [(0, n, (ref.avg4(total, n, 0), 4), (total, 0))])


def test_growth_keeps_records(hip):
    """20,000 groups into a table hinted at 16, small and large chunks
    mixed: slot-indexed records move through the x4 rehash and the failed
    rows of an overflowing insert rerun exactly once."""
    rng = np.random.default_rng(2803)
    n = 275_000
    gk = rng.integers(0, 20_000, n, dtype=np.int64)
    vals = PALETTE[rng.integers(0, len(PALETTE), n)]
    nulls = (rng.random(n) < 0.05).astype(np.uint8)
    cuts = [0, 3000, 268_000, 270_000, n]
    chunks = [Chunk([Block(I64, values=gk[a:b]),
                     Block(I64, values=vals[a:b], nulls=nulls[a:b])])
              for a, b in zip(cuts, cuts[1:])]
    assert chunks[1].n_rows >= 1 << 18
    want = ref.ref_sum([(int(k),) for k in gk], pyvals(vals, nulls), 0)
    got = run(hip, [0], [(abi.sum_dec(0), 1)], [I64, I64], chunks,
              expected_groups=16)
    ref.same(got, ref.expected_rows(want))


def test_global_aggregate(hip):
    keys, pv, chunks, _ = carry_data()
    aggs = [(abi.sum_dec(0), 1), (abi.avg_dec(0), 1)]
    want = ref.expected_rows(ref.ref_sum(None, pv, 0),
                             ref.ref_avg(None, pv, 0))
    ref.same(run(hip, [], aggs, [I64, I64], chunks), want)
    # empty input: one NULL row
    ref.same(run(hip, [], aggs, [I64, I64], []), [(None, None)])
    # all-NULL input
    n = 2500
    allnull = chunks_from_columns(
        [I64, I64], [(np.zeros(n, dtype=np.int64), None),
                     (np.full(n, 5, dtype=np.int64),
                      np.ones(n, dtype=np.uint8))], chunk_size=997)
    ref.same(run(hip, [], aggs, [I64, I64], allnull), [(None, None)])


@pytest.mark.parametrize("scale", [2, 4, 9])
def test_i32_input_and_scales(hip, scale):
    """I32 values already scaled by 10^scale; the emitted record is checked
    byte-wise: fractions bytes and the left-aligned fraction word."""
    rng = np.random.default_rng(2804 + scale)
    n = 9000
    gk = rng.integers(0, 700, n, dtype=np.int64)
    vals = rng.integers(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype(np.int32)
    nulls = (rng.random(n) < 0.1).astype(np.uint8)
    chunks = chunks_from_columns([I64, I32], [(gk, None), (vals, nulls)],
                                 chunk_size=997)
    want = ref.ref_sum([(int(k),) for k in gk], pyvals(vals, nulls), scale)
    out = run_agg(hip, [0], [(abi.sum_dec(scale), 1)], [I64, I32], chunks,
                  device=0)
    ref.same(ref.result_rows(out), ref.expected_rows(want))
    checked = 0
    for c in out:
        assert c.blocks[1].type == DECIMAL
        for k, rec in c.rows():
            cell = want[(k,)]
            if cell is None:
                assert rec is None
                continue
            assert rec == dec40_encode_wide(cell[0], scale)
            assert rec[37] == scale and rec[38] == scale
            checked += 1
    assert checked > 600


def _dec_rows(rng, n, digit_choices, scale, null_frac=0.1):
    """Values with per-value fractions f <= scale (given at scale f) and
    their contribution at `scale`."""
    vals, fracs, contrib = [], [], []
    for _ in range(n):
        if rng.random() < null_frac:
            vals.append(None)
            fracs.append(0)
            contrib.append(None)
            continue
        f = int(rng.integers(0, scale + 1))
        digits = int(rng.choice(digit_choices))
        v = int(rng.integers(10 ** 8, 10 ** 9)) if digits <= 9 else \
            int("".join(str(int(d)) for d in rng.integers(1, 10, digits)))
        v %= 10 ** digits
        if rng.random() < 0.5:
            v = -v
        vals.append(v)
        fracs.append(f)
        contrib.append(v * 10 ** (scale - f))
    return vals, fracs, contrib


@pytest.mark.parametrize("digits,scale", [((9, 18), 2), ((19, 24, 27), 2),
                                          ((20, 28, 29), 0)])
def test_decimal_input(hip, digits, scale):
    """40-B records in: the simple 9- and 18-digit layouts, mixed per-value
    fractions, negatives, NULLs, and wide values of 3 to 4 integer words.
    Alone (fused insert), with more aggregates (accumulate pass), global."""
    rng = np.random.default_rng(2810 + scale + len(digits))
    n = 4000
    gk = rng.integers(0, 150, n, dtype=np.int64)
    vals, fracs, contrib = _dec_rows(rng, n, digits, scale)
    assert all(c is None or abs(c) < 10 ** 29 for c in contrib)
    if max(digits) > 18:   # 3 integer words; 28 digits and up: 4
        assert any(v is not None and abs(v) >= 10 ** 18 for v in vals)
    if max(digits) > 27:
        assert any(v is not None and abs(v) >= 10 ** 27 for v in vals)
    keys = [(int(k),) for k in gk]
    chunks = ref.split_chunks(
        lambda a, b: [Block(I64, values=gk[a:b]),
                      ref.dec_block(vals[a:b], scale_of=fracs[a:b])], n, 997)
    types = [I64, DECIMAL]
    want = ref.ref_sum(keys, contrib, scale)
    ref.same(run(hip, [0], [(abi.sum_dec(scale), 1)], types, chunks),
             ref.expected_rows(want))
    cnt = {}
    for k in keys:
        cnt[k] = cnt.get(k, 0) + 1
    ref.same(run(hip, [0], [(abi.COUNT_ROW, -1), (abi.MAX_I64, 0),
                            (abi.sum_dec(scale), 1), (abi.avg_dec(scale), 1)],
                 types, chunks),
             ref.expected_rows(cnt, {k: k[0] for k in cnt}, want,
                               ref.ref_avg(keys, contrib, scale)))
    ref.same(run(hip, [], [(abi.sum_dec(scale), 1)], types, chunks),
             ref.expected_rows(ref.ref_sum(None, contrib, scale)))


def test_two_phase_on_one_device(hip):
    """Partial SUM_DEC per shard, partial outputs concatenated, final agg
    through final_agg_specs == single phase. Partial sums pass 2^64, so the
    partial DECIMAL column is genuinely wide."""
    keys, pv, chunks, want = carry_data()
    partial_aggs = [(abi.sum_dec(0), 1), (abi.COUNT_COL, 1)]
    half = len(chunks) // 2
    partial_out = []
    for shard in (chunks[:half], chunks[half:]):
        partial_out += run_agg(hip, [0], partial_aggs, [I64, I64], shard,
                               device=0)
    wide = [abs(v[0]) for v in
            (c for r in ref.result_rows(partial_out) for c in r[1:2])
            if v is not None]
    assert max(wide) >= 2 ** 64
    finals, ftypes = final_agg_specs(1, partial_aggs)
    assert ftypes == [DECIMAL, I64]
    got = run(hip, [0], finals, [I64] + ftypes, partial_out)
    cnt = {}
    for k, v in zip(keys, pv):
        cnt[k] = cnt.get(k, 0) + (v is not None)
    ref.same(got, ref.expected_rows(want, cnt))
    single = run(hip, [0], partial_aggs, [I64, I64], chunks)
    ref.same(got, single)


def _record(words, integers, fractions):
    rec = np.zeros(40, dtype=np.uint8)
    rec[:4 * len(words)] = np.array(words, dtype="<i4").view(np.uint8)
    rec[36], rec[37], rec[38] = integers, fractions, fractions
    return rec


@pytest.mark.parametrize("bad,scale,fence", [
    (np.frombuffer(dec40_encode_wide(12345, 5), dtype=np.uint8), 2,
     "fractions fence"),
    (np.frombuffer(dec40_encode_wide(10 ** 29, 0), dtype=np.uint8), 0,
     "magnitude fence"),
    (np.frombuffer(dec40_encode_wide(10 ** 27, 0), dtype=np.uint8), 2,
     "magnitude fence"),
    (_record([1] * 9, 82, 0), 0, "words fence"),
])
@pytest.mark.parametrize("group_cols", [[0], []])
def test_fences(hip, bad, scale, fence, group_cols):
    """A value the device cannot bring to the aggregate's scale fails the
    consume with an error naming the fence; the process goes on and a valid
    op works afterwards."""
    n = 1200
    good = [i * 7 - 300 for i in range(n)]
    blk = ref.dec_block(good, scale=0)
    blk.values[777] = bad
    chunk = Chunk([Block(I64, values=np.arange(n, dtype=np.int64) % 11), blk])
    op = HashAggExec(hip, group_cols, [(abi.sum_dec(scale), 1)],
                     [I64, DECIMAL], device=0)
    try:
        with pytest.raises(RuntimeError, match=fence):
            op.consume_chunk(chunk)
    finally:
        op.close()
    ok = Chunk([Block(I64, values=np.arange(n, dtype=np.int64) % 11),
                ref.dec_block(good, scale=0)])
    keys = None if not group_cols else [(i % 11,) for i in range(n)]
    want = ref.ref_sum(keys, [g * 10 ** scale for g in good], scale)
    ref.same(run(hip, group_cols, [(abi.sum_dec(scale), 1)], [I64, DECIMAL],
                 [ok]), ref.expected_rows(want))


@pytest.mark.parametrize("scale", [0, 2, 4])
def test_avg_dec(hip, scale):
    """round_half_up(sum / count, 4): exact .5 ties in both signs (an odd
    sum over count = 2 x 10^(4-scale)), count = 1, a NULL group, a sum past
    2^64, plus random groups."""
    tie_count = 2 * 10 ** (4 - scale)
    keys, vals = [], []

    def group(k, vs):
        keys.extend([(k,)] * len(vs))
        vals.extend(vs)

    group(1, [3] + [0] * (tie_count - 1))            # +x.xxxx5 tie
    group(2, [-3] + [0] * (tie_count - 1))           # -x.xxxx5 tie
    group(3, [1] * (tie_count - 1) + [2])            # odd sum, all nonzero
    group(4, [12345])                                # count = 1
    group(5, [-1])
    group(6, [None, None, None])                     # NULL group
    group(7, [I64_MAX] * 5 + [None])                 # sum past 2^64
    group(8, [I64_MIN] * 6 + [1])
    group(9, [1, 1, None, 0])                        # 2/3 -> rounds up
    group(10, [-1, -1, 0])
    rng = np.random.default_rng(2820 + scale)
    for k in range(100, 400):
        m = int(rng.integers(1, 40))
        group(k, [int(x) for x in rng.integers(-10 ** 12, 10 ** 12, m)])
    order = rng.permutation(len(keys))
    keys = [keys[i] for i in order]
    vals = [vals[i] for i in order]
    want = ref.ref_avg(keys, vals, scale)
    assert want[(1,)] is not None and want[(6,)] is None
    gk = np.array([k[0] for k in keys], dtype=np.int64)
    nulls = np.array([v is None for v in vals], dtype=np.uint8)
    arr = np.array([0 if v is None else v for v in vals], dtype=np.int64)
    chunks = chunks_from_columns([I64, I64], [(gk, None), (arr, nulls)],
                                 chunk_size=997)
    aggs = [(abi.avg_dec(scale), 1), (abi.sum_dec(scale), 1)]
    ref.same(run(hip, [0], aggs, [I64, I64], chunks),
             ref.expected_rows(want, ref.ref_sum(keys, vals, scale)))
    # AVG alone: the 3-slot record on the slot-fused path
    ref.same(run(hip, [0], aggs[:1], [I64, I64], chunks),
             ref.expected_rows(want))


def _err(fn):
    with pytest.raises(RuntimeError) as e:
        fn()
    return str(e.value)


def test_create_rejections(hip):
    mk = lambda f, t=I64: HashAggExec(hip, [0], [(f, 1)], [I64, t], device=0)
    assert "scale 10" in _err(lambda: mk(abi.sum_dec(10)))
    assert "scale 300" in _err(lambda: mk(abi.sum_dec(300)))
    assert "scale 5" in _err(lambda: mk(abi.avg_dec(5)))
    assert "AVG_DEC" in _err(lambda: mk(abi.avg_dec(9)))
    for t in (SLICE, F64):
        msg = _err(lambda: mk(abi.sum_dec(0), t))
        assert "SUM_DEC" in msg and "input type" in msg
        assert "input type" in _err(lambda: mk(abi.avg_dec(0), t))
    assert "out of range" in _err(lambda: HashAggExec(
        hip, [0], [(abi.sum_dec(0), 2)], [I64, I64], device=0))
    # a scale on a func that takes none is no known func
    assert "unknown" in _err(lambda: mk(abi.with_scale(abi.SUM_I64N, 2)))
    # the accepted edge still creates
    mk(abi.sum_dec(9)).close()
    mk(abi.avg_dec(4), DECIMAL).close()


@pytest.mark.parametrize("func", [abi.sum_dec(0), abi.sum_dec(2),
                                  abi.avg_dec(0)])
def test_other_ops_reject_dec(hip, func):
    msg = _err(lambda: HashGroupJoinExec(
        hip, abi.INNER, [EquiJoinKey(0, 0, I64)], [I64], [I64, I64],
        group_cols=[0], aggs=[(func, 1)], device=0))
    assert "SUM_DEC/AVG_DEC" in msg and "group-join" in msg
    msg = _err(lambda: NonFrameOverWindowExec(
        hip, [0], [(func, 1)], [I64, I64], device=0))
    assert "SUM_DEC/AVG_DEC" in msg and "window" in msg
    msg = _err(lambda: OverWindowFramesExec(
        hip, [0], [(func, 1, abi.FRAME_WHOLE_PARTITION, 0, 0)], [I64, I64],
        device=0))
    assert "SUM_DEC/AVG_DEC" in msg and "frame-window" in msg


def test_driver_selftest_decsum():
    """tools/gx_driver selftest: 4096 x INT64_MAX into one group, the
    expected 40 bytes in closed form, and its NULL-group companion."""
    import os
    import subprocess
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run(["make", "-C", os.path.join(repo, "tools")], check=True,
                   capture_output=True)
    r = subprocess.run(
        [os.path.join(repo, "tools", "gx_driver"), "--lib",
         os.path.join(repo, "galaxysql_amd", "csrc", "libgxhip.so"),
         "--device", "0", "selftest"],
        capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "decsum" in r.stdout and "SELFTEST PASSED" in r.stdout
