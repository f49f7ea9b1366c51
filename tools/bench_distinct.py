"""A/B: COUNT(DISTINCT v) GROUP BY keys as ONE agg op with a distinct
aggregator vs the only alternative without it — the two-level rewrite as
two plain HashAggExec passes (GROUP BY keys, v  ->  GROUP BY keys,
COUNT_COL(v)) on the same HIP library, the intermediate staying on the
device.

Shapes:
  q16      16M rows, ~28k groups on three key columns (TPC-H Q16's
           p_brand x p_type x p_size), values uniform in [0, 100k)
  highcard 16M rows, 4M groups on one key, ~2 distinct values per group

Each shape runs twice: without a size hint (expected_groups=0: every table
starts at its minimum and grows x4 by overflow retry), then with
expected_groups set to the true cardinalities (a planner with perfect
estimates — the case most favourable to the rewrite, whose first pass has
one group per distinct pair).

Each variant: 2 warm-up runs, then 7 timed runs; the median wall time and
the median of the ops' HIP-event time (stats()["kernel_ms"]) are printed,
one JSON line per shape and round. Wall time covers create, consume, emit
and close; inputs are device-resident, so there is no PCIe transfer.

Run on an MI355X box:  python tools/bench_distinct.py [scale]
"""
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from galaxysql_amd import abi
from galaxysql_amd.chunk import I64, I32
from galaxysql_amd.operators import HashAggExec

WARMUP, REPEATS = 2, 7

# Distinct pass, algorithmic bytes per input row (fixed-width value):
#   pack:   value read 8 + slot_of_row read 4 + slots[].gid read 16 (random)
#           + record write 16 + status write 1
#   insert: status read 1 + record read 16 + slot line 8 (random, CAS when
#           empty) + owner record 16 (random, only when the tag matches)
#           + status write 1
#   winner only: RMW on records[gid] (8 per distinct agg)
DISTINCT_BYTES_PER_ROW = (8 + 4 + 16 + 16 + 1) + (1 + 16 + 8 + 16 + 1)


def dev_chunk(cols, types):
    return [{"type": t, "values": c.data_ptr(), "n_rows": c.numel()}
            for c, t in zip(cols, types)]


def consume_dev(lib, op, cols, types, keep):
    gc = lib.to_gx_chunk(None, keep, device_ptrs=dev_chunk(cols, types))
    lib.check(lib.lib.gxop_agg_consume(op._op, C.byref(gc)), "agg_consume")


def next_result(lib, op):
    out = C.POINTER(abi.GxResult)()
    lib.check(lib.lib.gxop_agg_next(op._op, C.byref(out)), "agg_next")
    return out


def run_single(lib, cols, types, nk, hints):
    """One op: GROUP BY keys, COUNT_DISTINCT(v). Returns (wall s, kernel ms,
    groups, sum of counts). hints = (groups, pairs) or None."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    op = HashAggExec(lib, list(range(nk)), [(abi.COUNT_DISTINCT, nk)], types,
                     expected_groups=hints[0] if hints else 0, device=0)
    keep = []
    consume_dev(lib, op, cols, types, keep)
    op.build_consume()
    out = next_result(lib, op)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    kms = op.stats()["kernel_ms"]
    groups = out.contents.chunk.n_rows
    cnt = torch.empty(groups, dtype=torch.int64, device="cuda:0")
    lib.check(lib.lib.gxop_result_copy_col(out, nk, C.c_void_p(cnt.data_ptr()),
                                           None), "copy_col")
    total = int(cnt.sum().item())
    lib.lib.gxop_result_release(out)
    op.close()
    return wall, kms, groups, total


def run_rewrite(lib, cols, types, nk, hints):
    """Two plain ops: GROUP BY (keys, v) COUNT_ROW, then GROUP BY keys
    COUNT_COL(v) over the device-resident result of the first."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    op1 = HashAggExec(lib, list(range(nk + 1)), [(abi.COUNT_ROW, -1)], types,
                      expected_groups=hints[1] if hints else 0, device=0)
    keep = []
    consume_dev(lib, op1, cols, types, keep)
    op1.build_consume()
    mid = next_result(lib, op1)
    op2 = HashAggExec(lib, list(range(nk)), [(abi.COUNT_COL, nk)],
                      list(types) + [I64],
                      expected_groups=hints[0] if hints else 0, device=0)
    lib.check(lib.lib.gxop_agg_consume(op2._op, C.byref(mid.contents.chunk)),
              "agg_consume")
    op2.build_consume()
    out = next_result(lib, op2)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    kms = op1.stats()["kernel_ms"] + op2.stats()["kernel_ms"]
    groups = out.contents.chunk.n_rows
    cnt = torch.empty(groups, dtype=torch.int64, device="cuda:0")
    lib.check(lib.lib.gxop_result_copy_col(out, nk, C.c_void_p(cnt.data_ptr()),
                                           None), "copy_col")
    total = int(cnt.sum().item())
    lib.lib.gxop_result_release(out)
    lib.lib.gxop_result_release(mid)
    op2.close()
    op1.close()
    return wall, kms, groups, total


def measure(fn, *args):
    for _ in range(WARMUP):
        fn(*args)
    runs = [fn(*args) for _ in range(REPEATS)]
    return (statistics.median(r[0] for r in runs) * 1e3,
            statistics.median(r[1] for r in runs), runs[0][2], runs[0][3])


def main():
    scale = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
    n = int(16_000_000 * scale)
    lib = abi.load_hip()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(16)

    def rnd(hi, dtype=torch.int64):
        return torch.randint(0, hi, (n,), device=dev, generator=g, dtype=dtype)

    truth = {}
    hk = rnd(int(4_000_000 * scale) or 1)
    shapes = {
        # 25 brands x 150 types x 8 sizes = 30k possible groups
        "q16": ([rnd(25, torch.int32), rnd(150, torch.int32),
                 rnd(8, torch.int32), rnd(100_000)], [I32, I32, I32, I64], 3),
        "highcard": ([hk, hk * 3 + rnd(2)], [I64, I64], 1),
    }

    # two rounds per shape: no size hint (both tables start at their minimum
    # and grow x4 by overflow retry), then expected_groups set to the true
    # cardinalities of the first round — the group count for GROUP BY keys,
    # the pair count for the rewrite's GROUP BY (keys, v) — i.e. a planner
    # with perfect estimates, the case most favourable to the rewrite
    for name, hinted in [(nm, h) for nm in shapes for h in (False, True)]:
        cols, types, nk = shapes[name]
        hints = truth[name] if hinted else None
        s_wall, s_k, s_groups, s_total = measure(run_single, lib, cols, types,
                                                 nk, hints)
        r_wall, r_k, r_groups, r_total = measure(run_rewrite, lib, cols, types,
                                                 nk, hints)
        assert (s_groups, s_total) == (r_groups, r_total), \
            f"{name}: single {s_groups}/{s_total} vs rewrite {r_groups}/{r_total}"
        truth[name] = (s_groups, s_total)
        print(json.dumps({
            "shape": name, "size_hints": hinted, "rows": n,
            "groups": s_groups,
            "distinct_pairs": s_total,
            "single_wall_ms": round(s_wall, 3),
            "single_kernel_ms": round(s_k, 3),
            "single_rows_per_s": round(n / (s_wall * 1e-3)),
            "rewrite_wall_ms": round(r_wall, 3),
            "rewrite_kernel_ms": round(r_k, 3),
            "rewrite_rows_per_s": round(n / (r_wall * 1e-3)),
            "wall_ratio_single_over_rewrite": round(s_wall / r_wall, 3),
            "kernel_ratio_single_over_rewrite": round(s_k / r_k, 3),
            "distinct_pass_model_bytes_per_row": DISTINCT_BYTES_PER_ROW,
            "warmup": WARMUP, "repeats": REPEATS}), flush=True)


if __name__ == "__main__":
    main()
