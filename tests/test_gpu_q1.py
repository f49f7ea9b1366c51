"""The TPC-H Q1 chain (queries.run_q1: scan -> low-cardinality hash
aggregation -> sort) against Python integers, and the GX_PROJ_Q1_CHARGE6
scan projection on its own and handed to the fused probe-scan."""
import ctypes as C

import numpy as np
import pytest

from galaxysql_amd import abi, queries
from galaxysql_amd.abi import GxResult
from galaxysql_amd.chunk import Block, Chunk, I32, I64
from galaxysql_amd.operators import (EquiJoinKey, ParallelHashJoinExec,
                                     ScanExec)

from . import decsum_ref as ref
from .test_gpu_probe_scan import canon, dev_chunk, same

pytestmark = pytest.mark.gpu

N = 300_000


@pytest.fixture(scope="module")
def hip():
    return abi.load_hip()


@pytest.fixture(scope="module")
def q1_data():
    cols = queries.gen_q1_numpy(np.random.default_rng(4101), N, nulls=True)
    return cols, queries.ref_q1_numpy(cols)


@pytest.mark.parametrize("local", [None, "1", "0"])
def test_run_q1(hip, monkeypatch, q1_data, local):
    """100,000-row chunks: three consumes of ~96,000 kept rows each, below
    the 2^18-row gate but past the 2^16-row one for few groups, so they go
    local unset and with GX_AGG_LOCAL=1 and through the plain kernel with
    =0. Exact every way."""
    if local is None:
        monkeypatch.delenv("GX_AGG_LOCAL", raising=False)
    else:
        monkeypatch.setenv("GX_AGG_LOCAL", local)
    cols, want = q1_data
    chunks, info = queries.run_q1(hip, 0, cols, chunk_rows=100_000)
    got = ref.result_rows(chunks)      # ORDER BY order, DECIMAL decoded
    assert len(want) == 4
    assert got == want
    assert info["lineitem_kept"] == sum(r[-1] for r in want)
    assert info["local_rows"] == (0 if local == "0"
                                  else info["lineitem_kept"])
    assert info["agg_kernel_ms"] > 0


def test_run_q1_small_chunks_below_the_gate(hip, monkeypatch, q1_data):
    """20,000-row chunks stay on the plain kernel when the switch is unset."""
    monkeypatch.delenv("GX_AGG_LOCAL", raising=False)
    cols, want = q1_data
    chunks, info = queries.run_q1(hip, 0, cols, chunk_rows=20_000)
    assert ref.result_rows(chunks) == want
    assert info["local_rows"] == 0


def test_run_q1_one_chunk_auto_gate(hip, monkeypatch, q1_data):
    """The whole table as one chunk passes the automatic gate."""
    monkeypatch.delenv("GX_AGG_LOCAL", raising=False)
    cols, want = q1_data
    chunks, info = queries.run_q1(hip, 0, cols, chunk_rows=N)
    assert ref.result_rows(chunks) == want
    assert info["lineitem_kept"] >= 1 << 18
    assert info["local_rows"] == info["lineitem_kept"]


CH_TYPES = [I64, I64, I64, I64]     # key, price cents, disc, tax
CH_PROJS = [(abi.PROJ_COPY, 0), (abi.PROJ_Q1_CHARGE6, 1, 2, 3)]


def charge_cols(n=10_000, seed=4102):
    rng = np.random.default_rng(seed)
    key = rng.integers(0, 300, n).astype(np.int64) * 3 + 1
    price = rng.integers(90_000, 10_500_000, n).astype(np.int64)
    disc = rng.integers(0, 11, n).astype(np.int64)
    tax = rng.integers(0, 9, n).astype(np.int64)
    nl = [(rng.random(n) < 0.07).astype(np.uint8) for _ in range(3)]
    return [(key, None), (price, nl[0]), (disc, nl[1]), (tax, nl[2])]


def test_charge_projection(hip):
    cols = charge_cols()
    s = ScanExec(hip, [], CH_PROJS, CH_TYPES, device=0)
    try:
        out = s.consume_chunk(Chunk([Block(t, values=v, nulls=nl)
                                     for t, (v, nl) in zip(CH_TYPES, cols)]))
    finally:
        s.close()
    (k, _), (p, pn), (d, dn), (t, tn) = cols
    want_null = pn | dn | tn
    assert want_null.any() and not want_null.all()
    assert [b.type for b in out.blocks] == [I64, I64]
    # the scan does not keep row order: compare as sorted (key, null, value)
    want = Chunk([Block(I64, values=k),
                  Block(I64, values=p * (100 - d) * (100 + t),
                        nulls=want_null)])
    assert out.n_rows == len(p)
    assert same(canon(out, 2), canon(want, 2))


def test_charge_projection_bad_column(hip):
    with pytest.raises(RuntimeError, match="bad scan projection"):
        ScanExec(hip, [], [(abi.PROJ_Q1_CHARGE6, 1, 2, 9)], CH_TYPES,
                 device=0)


def test_probe_scan_refuses_charge(hip):
    """An INNER join on one I64 key that the fused probe-scan would take:
    with a Q1_CHARGE6 projection in the scan it must run scan-then-probe
    (the fused gather has no wiring for the op), so both give the same
    rows, and the charge column is the expression's value."""
    cols = charge_cols()
    bkeys = np.arange(200, dtype=np.int64) * 3 + 1
    build = Chunk([Block(I64, values=bkeys),
                   Block(I32, values=np.arange(200, dtype=np.int32))])
    j = ParallelHashJoinExec(hip, abi.INNER, [EquiJoinKey(0, 0, I64)],
                             [I64, I64], [I64, I32], device=0)
    s = ScanExec(hip, [(2, abi.LE, 8)], CH_PROJS, CH_TYPES, device=0)
    try:
        j.consume_chunk(build)
        j.build_consume()
        ka = []
        gc = dev_chunk(hip, cols, CH_TYPES, ka)
        out, kept_a = j.probe_scan(s, C.byref(gc))
        chunk_a = hip.result_to_chunk(out)
        t = s.consume_raw(C.byref(gc))
        kept_b = t.contents.chunk.n_rows
        out = C.POINTER(GxResult)()
        hip.check(hip.lib.gxop_join_probe(j._op, C.byref(t.contents.chunk),
                                          C.byref(out)), "join_probe")
        chunk_b = hip.result_to_chunk(out)
        hip.lib.gxop_result_release(t)
    finally:
        j.close()
        s.close()
    assert kept_a == kept_b > 0 and chunk_b.n_rows > 1000
    assert same(canon(chunk_a, 4), canon(chunk_b, 4))
    # the values themselves: recompute from the raw columns by key multiset
    (k, _), (p, pn), (d, dn), (t_, tn) = cols
    keep = (dn == 0) & (d <= 8) & np.isin(k, bkeys)
    nul = (pn | tn).astype(bool)[keep]
    want = np.where(nul, 0, (p * (100 - d) * (100 + t_))[keep])
    got_n = (chunk_a.blocks[1].nulls.astype(bool)
             if chunk_a.blocks[1].nulls is not None
             else np.zeros(chunk_a.n_rows, bool))
    got = np.where(got_n, 0, chunk_a.blocks[1].values)
    assert chunk_a.n_rows == int(keep.sum())
    assert np.array_equal(np.sort(got), np.sort(want))
    assert int(got_n.sum()) == int(nul.sum())
