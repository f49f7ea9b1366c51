"""Fused scan+probe, the parts its three-stage kernel can get wrong.

k_probe_scan streams R rows per lane per iteration (a wave's tile is 64*R
rows, a block's 256*R), ballot-compacts the survivors of predicates + NULL
key + bloom into a per-wave LDS queue, and walks the buckets for 64 queued
rows at a time. tests/test_gpu_probe_scan.py covers wave and block edges
at one row per lane, NULLs per column, join shapes, bucket overflow and the
pair-list retry; this file covers tile edges, queue carry-over between
iterations, drains inside an iteration, the queue's worst case, unaligned
column pointers and predicate sets other than one I32 compare.

Every case goes through run_case of test_gpu_probe_scan.py: fused vs
scan-then-probe on the HIP library vs the CPU oracle, exact sorted
multisets, and n_scan_kept.
"""
import ctypes as C

import numpy as np
import pytest

from galaxysql_amd import abi
from galaxysql_amd.chunk import Block, I64, SLICE
from galaxysql_amd.operators import (ParallelHashJoinExec, ScanExec,
                                     EquiJoinKey)
from .test_gpu_probe_scan import (run_case, gen_raw, gen_build, canon,
                                  host_chunk, same, PRED_CUT, BIG_BUILD,
                                  RAW_TYPES, PROJS, OUT_TYPES, BUILD_TYPES)

pytestmark = pytest.mark.gpu

# mirrors of the kernel's compile-time shape (gxhip_scan.inc: GX_PS_R,
# GX_PS_TILE, GX_PS_BLOCK_ROWS, GX_PS_GRID_CAP)
R = 2
T = 64 * R              # rows per wave per iteration
B = 256 * R             # rows per block per iteration
G = 4096 * B            # rows one pass of the full grid covers

HALF = [(1, abi.GT, PRED_CUT["half"])]

# the big cases keep the compared rows narrow: probe key and date, build
# payload (the other projections are evaluated per matched row by
# k_gather_proj, which is not what these cases are about)
NARROW = [0, 3, 5]


@pytest.fixture(scope="module")
def small_build():
    return gen_build(np.random.default_rng(8001), 300)


@pytest.fixture(scope="module")
def big_build():
    return gen_build(np.random.default_rng(8002), BIG_BUILD)


@pytest.mark.parametrize("nulls", ["nulls", "nullfree"])
@pytest.mark.parametrize("n", [T - 1, T, T + 1, B - 1, B, B + 1, 3 * B + 17])
def test_tile_edges(n, nulls, small_build):
    """Last tile of a wave / of a block full, one short, one over."""
    rng = np.random.default_rng(1000 + n)
    build = small_build if nulls == "nulls" else \
        gen_build(np.random.default_rng(8003), 300, with_nulls=False)
    raw = gen_raw(rng, n, 300, "all", (0, 1, 2, 3, 4, 5)
                  if nulls == "nulls" else ())
    assert run_case(raw, build, HALF, null_free=(nulls == "nullfree")) > 0


@pytest.mark.parametrize("bloom", [0, 1])
@pytest.mark.parametrize("pred,match", [("half", "tenth"), ("all", "all")])
def test_queue_carry_over(pred, match, bloom, big_build):
    """n just above one pass of the full grid: the first T + 3 rows' waves
    run a second iteration and carry queued survivors into it.
    half/tenth: sparse queue, drains are rare, NULL keys and dates.
    all/all: the queue fills in every iteration and the emit stage flushes
    inside the drains. Without the bloom the input is null-free: every row
    survives, 64*R queued and R drains per iteration. With it 7 % of the
    keys are NULL: an iteration queues a little under 64*R on top of a
    carried remainder of up to 63."""
    n = G + T + 3
    rng = np.random.default_rng(1100 + bloom)
    if pred == "half":
        nulls, out_proj = (0, 1), NARROW
    else:
        nulls, out_proj = ((0,) if bloom else ()), [0, 5]
    raw = gen_raw(rng, n, BIG_BUILD, match, nulls)
    rows = run_case(raw, big_build, [(1, abi.GT, PRED_CUT[pred])],
                    out_proj=out_proj, enable_bloom=bool(bloom))
    assert rows > 0


def test_queue_worst_case():
    """Every row survives, no bloom, build keys duplicated 6x (overflow
    runs), INNER: each wave queues 64*R rows and drains R times inside the
    iteration; 6 pairs per row fill the 384-pair emit stage in every
    drain and the first-attempt pair list (2n), forcing the exact-size
    retry from inside a drain."""
    rng = np.random.default_rng(1200)
    n = 24 * B + 17
    build = gen_build(rng, 500, dup=6, with_nulls=False)
    raw = gen_raw(rng, n, 500, "all", ())
    assert run_case(raw, build, [(1, abi.GT, PRED_CUT["all"])]) == 6 * n


def test_semi_duplicates():
    """SEMI over build keys duplicated 3x: a surviving probe row comes out
    exactly once."""
    rng = np.random.default_rng(1300)
    n = 5 * B + 77
    build = gen_build(rng, 400, dup=3)
    raw = gen_raw(rng, n, 400, "all", (0, 1))
    rows = run_case(raw, build, HALF, join_type=abi.SEMI)
    assert 0 < rows < n


@pytest.mark.parametrize("pred,match,bloom", [("none", "all", 0),
                                              ("all", "none", 1)])
def test_nothing_survives(pred, match, bloom, big_build):
    """The queue stays empty to the end; *kept is still right (run_case
    checks it against the composed scan's row count)."""
    rng = np.random.default_rng(1400 + bloom)
    raw = gen_raw(rng, 3 * B + 17, BIG_BUILD, match, (0, 1))
    assert run_case(raw, big_build, [(1, abi.GT, PRED_CUT[pred])],
                    enable_bloom=bool(bloom)) == 0


def dev_chunk_shifted(lib, cols, types, ka, shift):
    """dev_chunk of test_gpu_probe_scan.py for fixed-width columns, with
    `shift` extra leading elements uploaded and tensor[shift:] passed: at
    shift = 1 the value pointers are aligned to their element size only
    (8 B / 4 B, not 16 B) and the null-byte pointers to 1 B."""
    import torch

    def up(a):
        a = np.ascontiguousarray(a)
        t = torch.from_numpy(np.concatenate([a[:shift], a])).cuda()
        ka.append(t)
        return t[shift:].data_ptr()

    ptrs = []
    for c, ty in zip(cols, types):
        d = {"type": ty, "n_rows": len(c[0]), "values": up(c[0])}
        if c[1] is not None:
            d["nulls"] = up(c[1])
        ptrs.append(d)
    return lib.to_gx_chunk(None, ka, device_ptrs=ptrs)


def test_unaligned_views(big_build):
    """tensor[1:] views of every raw column: same rows and the same
    n_scan_kept as the aligned upload, which run_case ties to the oracle."""
    rng = np.random.default_rng(1500)
    n = 3 * B + 17
    raw = gen_raw(rng, n, BIG_BUILD, "tenth", (0, 1, 2, 3, 4, 5))
    assert run_case(raw, big_build, HALF, enable_bloom=True) > 0
    hip = abi.load_hip()
    got = []
    for shift in (0, 1):
        j = ParallelHashJoinExec(hip, abi.INNER, [EquiJoinKey(0, 0, I64)],
                                 OUT_TYPES, BUILD_TYPES, device=0,
                                 enable_bloom=True)
        s = ScanExec(hip, HALF, PROJS, RAW_TYPES, device=0)
        try:
            j.consume_chunk(host_chunk(big_build, BUILD_TYPES))
            j.build_consume()
            ka = []
            gc = dev_chunk_shifted(hip, raw, RAW_TYPES, ka, shift)
            if shift:
                assert gc.blocks[0].values % 16 == 8
                assert gc.blocks[1].values % 16 == 4
            out, kept = j.probe_scan(s, C.byref(gc))
            got.append((canon(hip.result_to_chunk(out),
                              len(OUT_TYPES) + len(BUILD_TYPES)), kept))
        finally:
            j.close()
            s.close()
    assert got[0][1] == got[1][1]
    assert got[0][0].shape[0] > 0 and same(got[0][0], got[1][0])


def test_two_predicates(small_build):
    """I32 and F64 predicates AND-ed, NULLs in both columns."""
    rng = np.random.default_rng(1600)
    raw = gen_raw(rng, 3 * B + 17, 300, "all", (0, 1, 2))
    preds = [(1, abi.GT, PRED_CUT["half"]), (2, abi.LT, 50000.0)]
    assert run_case(raw, small_build, preds) > 0


def test_i64_predicate_on_key(small_build):
    """One I64 predicate on the key column itself."""
    rng = np.random.default_rng(1601)
    raw = gen_raw(rng, 3 * B + 17, 300, "all", (0, 1))
    assert run_case(raw, small_build, [(0, abi.LE, 3 * 150 + 1)]) > 0


def test_slice_contains_predicate(small_build):
    """SLICE CONTAINS takes the per-row evaluation inside the R-row
    structure; the SLICE column is read by the predicate only."""
    rng = np.random.default_rng(1602)
    n = 3 * B + 17
    raw = gen_raw(rng, n, 300, "all", (0, 1))
    tags = [None if rng.random() < 0.05 else "t%d" % rng.integers(0, 50)
            for _ in range(n)]
    raw.append(Block.of(SLICE, tags))
    preds = [(1, abi.GT, PRED_CUT["half"]), (6, abi.CONTAINS, "t1")]
    assert run_case(raw, small_build, preds,
                    raw_types=RAW_TYPES + [SLICE]) > 0
