"""Block-local (LDS) pre-aggregation of the HIP hash aggregation: the
accumulate pass of a gid-indexed op with few groups (k_agg_accumulate_local /
_dec). Every func, the 128-bit carry under replicas, the global aggregate,
growth past the local group cap, generic (SLICE) keys, an op with DISTINCT
aggregates, the narrow-state hint, the GX_AGG_LOCAL switch and the automatic
gate. References: the CPU oracle through run_agg, tests/decsum_ref.py for the
DECIMAL sums. 300,000 rows is the smallest chunk past the 2^18-row
large-chunk boundary; 997-row chunks take the inline-gid mode.

Every test reads HashAggExec.local_stats(), which a library without the
path does not export."""
import functools
import math

import numpy as np
import pytest

from galaxysql_amd import abi
from galaxysql_amd.chunk import (Block, Chunk, DECIMAL, F64, I32, I64, SLICE,
                                 chunks_from_columns, rows_of)
from galaxysql_amd.operators import HashAggExec, run_agg

from . import decsum_ref as ref
from . import distinct_ref as dr

pytestmark = pytest.mark.gpu

N = 300_000
I64_MAX, I64_MIN = 2 ** 63 - 1, -2 ** 63


@pytest.fixture(scope="module")
def hip():
    return abi.load_hip()


@pytest.fixture(scope="module")
def oracle():
    return abi.load_oracle()


def run_hip(hip, group_cols, aggs, types, chunks, **kw):
    """(result chunks, local_stats) of one op over `chunks`."""
    op = HashAggExec(hip, group_cols, aggs, types, device=0, **kw)
    try:
        for ch in chunks:
            op.consume_chunk(ch)
        op.build_consume()
        return op.result_chunks(), op.local_stats()
    finally:
        op.close()


def _cell_same(g, w):
    if isinstance(w, float) and isinstance(g, float):
        if w != w or g != g:
            return w != w and g != g
        if w == 0.0 or g == 0.0:       # MIN/MAX: -0.0 and +0.0 differ
            return (w == g and
                    math.copysign(1.0, w) == math.copysign(1.0, g))
        if math.isinf(w) or math.isinf(g):
            return w == g
        # the project's f64 tolerance (tests/test_gpu_fuzz.py _close)
        return abs(g - w) <= 1e-9 * max(1.0, abs(g), abs(w))
    return g == w and type(g) is type(w)


def same_rows(got, want, n_keys):
    """Rows keyed by their group key (unique per row): integer / bytes / NULL
    cells exactly, f64 cells at 1e-9 relative, NaN == NaN, signed zeros."""
    gd = {r[:n_keys]: r for r in got}
    wd = {r[:n_keys]: r for r in want}
    assert len(gd) == len(got) and len(wd) == len(want)
    assert gd.keys() == wd.keys()
    for k, w in wd.items():
        g = gd[k]
        assert len(g) == len(w)
        for i, (gc, wc) in enumerate(zip(g, w)):
            assert _cell_same(gc, wc), (k, i, gc, wc)


# ---- every func ------------------------------------------------------------

EVERY_TYPES = [I64, I64, I32, F64, F64]
EVERY_AGGS = [(abi.COUNT_ROW, -1), (abi.COUNT_COL, 2), (abi.SUM_I64, 2),
              (abi.SUM_I64N, 1), (abi.MIN_I64, 1), (abi.MAX_I64, 2),
              (abi.SUM_F64, 3), (abi.AVG_F64, 3), (abi.AVG_F64, 2),
              (abi.MIN_F64, 4), (abi.MAX_F64, 4), (abi.BIT_AND, 1),
              (abi.BIT_OR, 1), (abi.BIT_XOR, 2)]


def every_columns(n_groups=5, seed=3101, global_agg=False):
    """gk, a (I64, signed), b (I32, >= 0), c (F64, >= 0), d (F64 for
    MIN/MAX: NaN in group 1, only -0.0 / +0.0 in group 2). 10% NULLs; the
    last group's inputs are all NULL."""
    rng = np.random.default_rng(seed)
    gk = rng.integers(0, n_groups, N, dtype=np.int64)
    a = rng.integers(-2 ** 40, 2 ** 40, N, dtype=np.int64)
    b = rng.integers(0, 2 ** 31 - 1, N, dtype=np.int64).astype(np.int32)
    c = rng.random(N) * 1e6
    d = rng.standard_normal(N) * 1e3
    d[(gk == 1) & (rng.random(N) < 0.01)] = np.nan
    z = gk == 2
    d[z] = np.where(rng.random(int(z.sum())) < 0.5, -0.0, 0.0)
    cols = []
    for v in (a, b, c, d):
        nl = rng.random(N) < 0.1
        if not global_agg:
            nl |= gk == n_groups - 1
        cols.append((v, nl.astype(np.uint8)))
    return [(gk, None)] + cols


@functools.lru_cache(maxsize=None)
def every_data():
    cols = every_columns()
    d, gk = cols[4][0], cols[0][0]
    assert np.isnan(d[(gk == 1) & (cols[4][1] == 0)]).any()
    z = d[(gk == 2) & (cols[4][1] == 0)]
    assert np.signbit(z).any() and (~np.signbit(z)).any() and (z == 0).all()
    one = chunks_from_columns(EVERY_TYPES, cols, chunk_size=N)
    small = chunks_from_columns(EVERY_TYPES, cols, chunk_size=997)
    want = rows_of(run_agg(abi.load_oracle(), [0], EVERY_AGGS, EVERY_TYPES,
                           small, device=-1))
    assert len(want) == 5
    dead = [r for r in want if r[0] == 4][0]
    assert dead[1] > 0 and dead[2] == 0 and dead[4] is None
    assert dead[5] is None and dead[10] is None and dead[11] is None
    return one, small, want


@pytest.mark.parametrize("mode", ["one_chunk", "chunks_997"])
def test_every_func(hip, monkeypatch, mode):
    monkeypatch.setenv("GX_AGG_LOCAL", "1")
    one, small, want = every_data()
    chunks = one if mode == "one_chunk" else small
    out, st = run_hip(hip, [0], EVERY_AGGS, EVERY_TYPES, chunks)
    same_rows(rows_of(out), want, 1)
    assert st["local_rows"] == N
    assert st["local_launches"] == len(chunks)
    assert st["replicas"] >= 1 and st["local_groups_cap"] >= 5


def test_switch(hip, monkeypatch):
    """GX_AGG_LOCAL=0 and =1 give the same rows; integer cells are equal
    bit for bit, and with 0 nothing goes through the local kernel."""
    one, _, want = every_data()
    monkeypatch.setenv("GX_AGG_LOCAL", "0")
    off, st0 = run_hip(hip, [0], EVERY_AGGS, EVERY_TYPES, one)
    monkeypatch.setenv("GX_AGG_LOCAL", "1")
    on, st1 = run_hip(hip, [0], EVERY_AGGS, EVERY_TYPES, one)
    assert st0["local_rows"] == 0 and st0["local_launches"] == 0
    assert st1["local_rows"] == N
    same_rows(rows_of(off), want, 1)
    same_rows(rows_of(on), rows_of(off), 1)
    # DECIMAL columns exact as well
    chunk, want_dec = carry_data(4)
    aggs = [(abi.sum_dec(0), 1), (abi.avg_dec(0), 1), (abi.COUNT_ROW, -1)]
    monkeypatch.setenv("GX_AGG_LOCAL", "0")
    off, st0 = run_hip(hip, [0], aggs, [I64, I64], [chunk])
    monkeypatch.setenv("GX_AGG_LOCAL", "1")
    on, st1 = run_hip(hip, [0], aggs, [I64, I64], [chunk])
    assert st0["local_rows"] == 0 and st1["local_rows"] == N
    ref.same(ref.result_rows(on), ref.result_rows(off))
    ref.same(ref.result_rows(off), want_dec)


# ---- 128-bit carry under replicas -----------------------------------------

@functools.lru_cache(maxsize=None)
def carry_data(n_groups):
    """test_gpu_decsum.py::test_one_hot_group's values: INT64_MAX and
    INT64_MIN+1 shuffled (they cancel), then a tail of INT64_MAX that takes
    the sum past 2^64; rows dealt round-robin to n_groups groups."""
    rng = np.random.default_rng(3102)
    half, tail = 149_500, 1000
    body = np.concatenate([np.full(half, I64_MAX, dtype=np.int64),
                           np.full(half, I64_MIN + 1, dtype=np.int64)])
    rng.shuffle(body)
    vals = np.concatenate([body, np.full(tail, I64_MAX, dtype=np.int64)])
    assert len(vals) == N
    gk = np.arange(N, dtype=np.int64) % n_groups
    keys = [(int(k),) for k in gk]
    pv = [int(v) for v in vals]
    sums = ref.ref_sum(keys, pv, 0)
    assert any(abs(c[0]) > 2 ** 64 for c in sums.values())
    cnt = {(g,): int((gk == g).sum()) for g in range(n_groups)}
    want = ref.expected_rows(sums, ref.ref_avg(keys, pv, 0), cnt)
    return Chunk([Block(I64, values=gk), Block(I64, values=vals)]), want


@pytest.mark.parametrize("n_groups", [1, 4])
def test_dec_carry_under_replicas(hip, monkeypatch, n_groups):
    monkeypatch.setenv("GX_AGG_LOCAL", "1")
    chunk, want = carry_data(n_groups)
    aggs = [(abi.sum_dec(0), 1), (abi.avg_dec(0), 1), (abi.COUNT_ROW, -1)]
    out, st = run_hip(hip, [0], aggs, [I64, I64], [chunk])
    ref.same(ref.result_rows(out), want)
    assert st["local_rows"] == N and st["replicas"] > 1


def test_dec_fence_message(hip, monkeypatch):
    """A GX_DECIMAL record the device cannot bring to the aggregate's scale
    fails the consume through the local kernel as through the plain one."""
    monkeypatch.setenv("GX_AGG_LOCAL", "1")
    from galaxysql_amd.chunk import dec40_encode_wide
    n = 1200
    blk = ref.dec_block([i * 7 - 300 for i in range(n)], scale=0)
    blk.values[777] = np.frombuffer(dec40_encode_wide(12345, 5),
                                    dtype=np.uint8)
    chunk = Chunk([Block(I64, values=np.arange(n, dtype=np.int64) % 3), blk])
    aggs = [(abi.sum_dec(2), 1), (abi.avg_dec(2), 1), (abi.COUNT_ROW, -1)]
    op = HashAggExec(hip, [0], aggs, [I64, DECIMAL], device=0)
    try:
        with pytest.raises(RuntimeError, match="fractions fence"):
            op.consume_chunk(chunk)
        assert op.local_stats()["local_launches"] == 1
    finally:
        op.close()


# ---- global aggregate -------------------------------------------------------

def test_global_aggregate(hip, oracle, monkeypatch):
    monkeypatch.setenv("GX_AGG_LOCAL", "1")
    cols = every_columns(global_agg=True)
    chunks = chunks_from_columns(EVERY_TYPES, cols, chunk_size=N)
    want = rows_of(run_agg(oracle, [], EVERY_AGGS, EVERY_TYPES, chunks,
                           device=-1))
    out, st = run_hip(hip, [], EVERY_AGGS, EVERY_TYPES, chunks)
    same_rows(rows_of(out), want, 0)
    assert st["local_rows"] == N
    # empty input: still one row, and nothing launched
    want = rows_of(run_agg(oracle, [], EVERY_AGGS, EVERY_TYPES, [],
                           device=-1))
    out, st = run_hip(hip, [], EVERY_AGGS, EVERY_TYPES, [])
    assert len(want) == 1
    same_rows(rows_of(out), want, 0)
    assert st["local_rows"] == 0 and st["local_launches"] == 0


# ---- growth past the cap ----------------------------------------------------

def test_growth_past_cap(hip, oracle, monkeypatch):
    """4 groups, then cap + 1000 groups, then 4 again: only the first chunk
    fits the local kernel; the state layout is the same, so the later chunks
    carry on in the plain kernel."""
    monkeypatch.setenv("GX_AGG_LOCAL", "1")
    aggs = [(abi.COUNT_ROW, -1), (abi.SUM_I64N, 1), (abi.MIN_I64, 1),
            (abi.MAX_I64, 1), (abi.BIT_XOR, 1)]
    types = [I64, I64]
    probe = HashAggExec(hip, [0], aggs, types, device=0)
    try:
        cap = probe.local_stats()["local_groups_cap"]
    finally:
        probe.close()
    assert 4 < cap < 4096
    rng = np.random.default_rng(3103)
    chunks = []
    for card in (4, cap + 1000, 4):
        gk = rng.integers(0, card, N, dtype=np.int64)
        gk[:card] = np.arange(card)       # every group present
        v = rng.integers(-2 ** 40, 2 ** 40, N, dtype=np.int64)
        nl = (rng.random(N) < 0.1).astype(np.uint8)
        chunks.append(Chunk([Block(I64, values=gk),
                             Block(I64, values=v, nulls=nl)]))
    want = rows_of(run_agg(oracle, [0], aggs, types, chunks, device=-1))
    out, st = run_hip(hip, [0], aggs, types, chunks)
    assert len(want) == cap + 1000
    same_rows(rows_of(out), want, 1)
    assert st["local_rows"] == N and st["local_launches"] == 1


# ---- SLICE keys, DISTINCT op ------------------------------------------------

def test_slice_group_keys(hip, oracle, monkeypatch):
    monkeypatch.setenv("GX_AGG_LOCAL", "1")
    rng = np.random.default_rng(3104)
    code = rng.integers(0, 6, N)
    data = np.frombuffer(b"ANRFOX", dtype=np.uint8)[code].copy()
    keys = Block(SLICE, offsets=np.arange(1, N + 1, dtype=np.int32),
                 data=data)
    v = rng.integers(-2 ** 40, 2 ** 40, N, dtype=np.int64)
    c = rng.random(N)
    nl = (rng.random(N) < 0.1).astype(np.uint8)
    chunk = Chunk([keys, Block(I64, values=v, nulls=nl),
                   Block(F64, values=c, nulls=nl)])
    types = [SLICE, I64, F64]
    aggs = [(abi.COUNT_ROW, -1), (abi.SUM_I64N, 1), (abi.MAX_I64, 1),
            (abi.SUM_F64, 2), (abi.AVG_F64, 2)]
    want = rows_of(run_agg(oracle, [0], aggs, types, [chunk], device=-1))
    out, st = run_hip(hip, [0], aggs, types, [chunk])
    assert len(want) == 6
    same_rows(rows_of(out), want, 1)
    assert st["local_rows"] == N


def test_distinct_op_plain_aggs_go_local(hip, oracle, monkeypatch):
    monkeypatch.setenv("GX_AGG_LOCAL", "1")
    rng = np.random.default_rng(3105)
    gk = rng.integers(0, 3, N, dtype=np.int64)
    x = rng.integers(0, 5000, N, dtype=np.int64)
    y = rng.integers(-2 ** 40, 2 ** 40, N, dtype=np.int64)
    nl = (rng.random(N) < 0.1).astype(np.uint8)
    chunk = Chunk([Block(I64, values=gk), Block(I64, values=x, nulls=nl),
                   Block(I64, values=y, nulls=nl)])
    types = [I64, I64, I64]
    aggs = [(abi.COUNT_DISTINCT, 1), (abi.SUM_I64, 2), (abi.MIN_I64, 2)]
    # the oracle runs DISTINCT through the two-level rewrite
    want = dr.rewrite_agg(oracle, [0], aggs, types, [chunk])
    out, st = run_hip(hip, [0], aggs, types, [chunk])
    assert len(want) == 3
    same_rows(rows_of(out), [tuple(r) for r in want], 1)
    assert st["local_rows"] == N


# ---- narrow state and the hint; the automatic gate -------------------------

def test_narrow_state_hint(hip, oracle, monkeypatch):
    """COUNT + SUM is a 2-slot record: slot-fused by default, gid-indexed
    and block-local with a hint of few groups."""
    monkeypatch.delenv("GX_AGG_LOCAL", raising=False)
    rng = np.random.default_rng(3106)
    gk = rng.integers(0, 4, N, dtype=np.int64)
    v = rng.integers(-2 ** 40, 2 ** 40, N, dtype=np.int64)
    chunk = Chunk([Block(I64, values=gk), Block(I64, values=v)])
    aggs = [(abi.COUNT_ROW, -1), (abi.SUM_I64, 1)]
    want = rows_of(run_agg(oracle, [0], aggs, [I64, I64], [chunk],
                           device=-1))
    out, st = run_hip(hip, [0], aggs, [I64, I64], [chunk], expected_groups=4)
    same_rows(rows_of(out), want, 1)
    assert st["local_rows"] == N
    out, st = run_hip(hip, [0], aggs, [I64, I64], [chunk], expected_groups=0)
    same_rows(rows_of(out), want, 1)
    assert st["local_rows"] == 0


def test_auto_gate(hip, monkeypatch):
    """Unset: a wide-state 4-group chunk of 300,000 rows goes local, one of
    1,000 rows does not. Between the two gates (2^16 <= rows < 2^18) a
    chunk goes local with few groups (<= 128) and not with more."""
    monkeypatch.delenv("GX_AGG_LOCAL", raising=False)
    chunk, want = carry_data(4)
    aggs = [(abi.sum_dec(0), 1), (abi.avg_dec(0), 1), (abi.COUNT_ROW, -1)]
    out, st = run_hip(hip, [0], aggs, [I64, I64], [chunk])
    ref.same(ref.result_rows(out), want)
    assert st["local_rows"] == N

    def head(n, n_groups):
        v = chunk.blocks[1].values[:n]
        return Chunk([Block(I64, values=np.arange(n, dtype=np.int64)
                            % n_groups), Block(I64, values=v)])

    for n, n_groups, local in ((1000, 4, False), (70_000, 4, True),
                               (70_000, 128, True), (70_000, 129, False),
                               (65_535, 4, False)):
        out, st = run_hip(hip, [0], aggs, [I64, I64], [head(n, n_groups)])
        assert sum(c.n_rows for c in out) == n_groups
        assert st["local_rows"] == (n if local else 0), (n, n_groups)
        counts = sorted(r[3] for r in rows_of(out))
        assert sum(counts) == n and counts[-1] - counts[0] <= 1
