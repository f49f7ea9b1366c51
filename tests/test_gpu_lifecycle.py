"""Device memory stays flat across operator lifecycles.

Every operator with a Python wrapper runs create -> consume -> build ->
probe/next -> result release -> close over and over on host (numpy) chunks
of 2^17 I64 rows, so the library stages the input itself and every
row-proportional device buffer (staged columns, stores, tables, index
lists, results) falls in a DevPool size class of at least 1 MiB.

The cap is derived, not measured: one row-proportional buffer leaked per
cycle costs >= 1 MiB x 32 cycles = 32 MiB per window; the cap is half of
that. The minimum over two windows tolerates one foreign allocation on a
shared card. Leaks of the small fixed-size buffers are below this test's
resolution; DevBuf's deleted copy constructor and its destructor cover
those at compile time.
"""
import ctypes as C

import numpy as np
import pytest

from galaxysql_amd import abi
from galaxysql_amd.abi import GxResult
from galaxysql_amd.chunk import Block, Chunk, I64, SLICE
from galaxysql_amd.operators import (
    EquiJoinKey, HashAggExec, HashGroupJoinExec, NonFrameOverWindowExec,
    OverWindowFramesExec, ParallelHashJoinExec, PartitioningExchanger,
    ScanExec)

pytestmark = pytest.mark.gpu

N = 1 << 17
WARMUP, WINDOW = 4, 32
CAP_BYTES = 16 << 20


def _i64(vals):
    return Block(I64, values=np.ascontiguousarray(vals, dtype=np.int64))


def _slice4():
    """N four-byte strings"""
    return Block(SLICE, offsets=(np.arange(1, N + 1) * 4).astype(np.int32),
                 data=np.arange(N, dtype=np.uint32).view(np.uint8).copy())


@pytest.fixture(scope="module")
def hip():
    return abi.load_hip()


@pytest.fixture(scope="module")
def data():
    ids = np.arange(N, dtype=np.int64)
    return {
        "ids": _i64(ids),
        "ids_hi": _i64(ids + N),
        "half": _i64(ids // 2),          # matches the lower half of ids
        "parts": _i64(ids // 64),        # sorted partition key
        "vals": _i64(ids % 1000),
        "text": _slice4(),
    }


def cycle_join(hip, d):
    """build_outer LEFT join with a SLICE payload; half the build rows stay
    unmatched and drain through tail"""
    op = ParallelHashJoinExec(hip, abi.LEFT, [EquiJoinKey(0, 0, I64)],
                              [I64, SLICE], [I64], build_outer=True, device=0)
    op.consume_chunk(Chunk([d["ids"], d["text"]]))
    op.build_consume()
    out = op.probe_chunk(Chunk([d["half"]]))
    tail = op.tail_chunks()
    op.close()
    assert out.n_rows == N
    assert sum(c.n_rows for c in tail) == N // 2


def cycle_agg(hip, d):
    """the second chunk doubles the group count: one rehash per cycle"""
    op = HashAggExec(hip, [0], [(abi.SUM_I64, 1), (abi.COUNT_ROW, -1)],
                     [I64, I64], device=0)
    op.consume_chunk(Chunk([d["ids"], d["vals"]]))
    op.consume_chunk(Chunk([d["ids_hi"], d["vals"]]))
    op.build_consume()
    out = op.result_chunks()
    op.close()
    assert sum(c.n_rows for c in out) == 2 * N


def cycle_part(hip, d):
    ch = Chunk([d["ids"], d["vals"]])
    op = PartitioningExchanger(hip, 8, [0], [I64, I64], device=0)
    outs = op.consume_chunk(ch)
    ka = []
    gc = hip.to_gx_chunk(ch, ka)
    res = C.POINTER(GxResult)()
    counts = (C.c_int64 * 8)()
    hip.check(hip.lib.gxop_part_consume_concat(op._op, C.byref(gc),
                                               C.byref(res), counts),
              "part_consume_concat")
    cat = hip.result_to_chunk(res)
    op.close()
    assert sum(c.n_rows for c in outs if c is not None) == N
    assert cat.n_rows == N and sum(counts) == N


def cycle_scan(hip, d):
    op = ScanExec(hip, [(1, abi.LT, 500)],
                  [(abi.PROJ_COPY, 0, -1), (abi.PROJ_COPY, 1, -1)],
                  [I64, I64], device=0)
    out = op.consume_chunk(Chunk([d["ids"], d["vals"]]))
    op.close()
    assert 0 < out.n_rows < N


def cycle_window(hip, d):
    op = NonFrameOverWindowExec(hip, [0], [(abi.SUM_I64, 1)],
                                [I64, I64, SLICE], device=0)
    out = op.consume_chunk(Chunk([d["parts"], d["vals"], d["text"]]))
    op.close()
    assert out.n_rows == N and len(out.blocks) == 4


def cycle_fwindow(hip, d):
    op = OverWindowFramesExec(
        hip, [0], [(abi.SUM_I64, 1, abi.FRAME_ROWS_SLIDING, 2, 2)],
        [I64, I64, SLICE], device=0)
    op.consume_chunk(Chunk([d["parts"], d["vals"], d["text"]]))
    op.finish()
    out = op.result_chunks()
    op.close()
    assert sum(c.n_rows for c in out) == N and len(out[0].blocks) == 4


def cycle_groupjoin(hip, d):
    op = HashGroupJoinExec(hip, abi.INNER, [EquiJoinKey(0, 0, I64)],
                           [I64, I64], [I64, I64], [0],
                           [(abi.SUM_I64, 1), (abi.COUNT_ROW, -1)], device=0)
    op.consume_chunk(Chunk([d["ids"], d["vals"]]))
    op.build_consume()
    op.probe_chunk(Chunk([d["half"], d["vals"]]))
    out = op.result_chunks()
    op.close()
    assert sum(c.n_rows for c in out) == N // 2


CYCLES = {"join": cycle_join, "agg": cycle_agg, "part": cycle_part,
          "scan": cycle_scan, "window": cycle_window,
          "fwindow": cycle_fwindow, "groupjoin": cycle_groupjoin}


@pytest.mark.parametrize("name", list(CYCLES))
def test_device_memory_flat_across_lifecycles(hip, data, name):
    import torch

    def free_bytes():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    cycle = CYCLES[name]
    for _ in range(WARMUP):
        cycle(hip, data)
    marks = [free_bytes()]
    for _ in range(2):
        for _ in range(WINDOW):
            cycle(hip, data)
        marks.append(free_bytes())
    drops = [marks[0] - marks[1], marks[1] - marks[2]]
    print(f"{name}: free-memory drop per {WINDOW}-cycle window = "
          f"{[x / 2**20 for x in drops]} MiB")
    assert min(drops) < CAP_BYTES
