"""A/B: what the exact DECIMAL sum costs. SUM_I64N (one wrapping u64, a
non-returning atomic add per row) against SUM_DEC(2) (128-bit state, one
RETURNING add per row plus a rare carry add) over the same device-resident
int64 column, one device.

Shapes (rows x scale):
  manygroups  100M rows -> 25M groups: bench.py's C4 aggregate (SUM of
              l_quantity GROUP BY l_orderkey, ~4 rows per group) scaled down;
              keys 4 x uniform, values 1..50 in hundredths
  fewgroups   100M rows -> 16 groups: every atomic lands on 16 hot records

Each shape: the two variants run ALTERNATELY (A, B, A, B, ...), 2 warm-up
runs each, then 7 timed runs each; medians and the min..max spread of wall
time and of the op's HIP-event time (stats()["kernel_ms"]) are printed, one
JSON line per shape. Wall time covers create, consume, emit and close. The
two results are compared on the device: same group count, same total.

Run on an MI355X box:  python tools/bench_decsum.py [scale]
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
from galaxysql_amd.chunk import I64
from galaxysql_amd.operators import HashAggExec

WARMUP, REPEATS = 2, 7
SCALE = 2  # decimal scale of the summed column (hundredths)


def run_one(lib, cols, func, groups_hint):
    """GROUP BY col 0, func(col 1). Returns (wall s, kernel ms, groups,
    total of the sums as a Python int)."""
    types = [I64, I64]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    op = HashAggExec(lib, [0], [(func, 1)], types,
                     expected_groups=groups_hint, device=0)
    keep = []
    gc = lib.to_gx_chunk(None, keep, device_ptrs=[
        {"type": I64, "values": c.data_ptr(), "n_rows": c.numel()}
        for c in cols])
    lib.check(lib.lib.gxop_agg_consume(op._op, C.byref(gc)), "agg_consume")
    op.build_consume()
    out = C.POINTER(abi.GxResult)()
    lib.check(lib.lib.gxop_agg_next(op._op, C.byref(out)), "agg_next")
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    kms = op.stats()["kernel_ms"]
    groups = out.contents.chunk.n_rows
    dev = cols[0].device
    if abi.base_func(func) == abi.SUM_DEC:
        rec = torch.empty((groups, 10), dtype=torch.int32, device=dev)
        lib.check(lib.lib.gxop_result_copy_col(
            out, 1, C.c_void_p(rec.data_ptr()), None), "copy_col")
        layout = rec[:, 9].contiguous().view(torch.uint8).view(groups, 4)
        words = (layout[:, 0] // 9).to(torch.int64)   # integer words
        assert int(words.max().item()) <= 2 and int(layout[:, 3].sum()) == 0
        w = rec.to(torch.int64)
        two = words == 2
        ip = torch.where(two, w[:, 0] * 10 ** 9 + w[:, 1], w[:, 0])
        fr = torch.where(two, w[:, 2], w[:, 1]) // 10 ** (9 - SCALE)
        total = int(ip.sum().item()) * 10 ** SCALE + int(fr.sum().item())
    else:
        s = torch.empty(groups, dtype=torch.int64, device=dev)
        lib.check(lib.lib.gxop_result_copy_col(
            out, 1, C.c_void_p(s.data_ptr()), None), "copy_col")
        total = int(s.sum().item())
    lib.lib.gxop_result_release(out)
    op.close()
    return wall, kms, groups, total


def spread(xs):
    return [round(min(xs), 3), round(statistics.median(xs), 3),
            round(max(xs), 3)]


def main():
    scale = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
    n = int(100_000_000 * scale)
    lib = abi.load_hip()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(28)
    vals = torch.randint(1, 51, (n,), device=dev, generator=g,
                         dtype=torch.int64) * 100
    shapes = {"manygroups": max(int(25_000_000 * scale), 1), "fewgroups": 16}
    variants = [("sum_i64n", abi.SUM_I64N), ("sum_dec", abi.sum_dec(SCALE))]
    for name, n_groups in shapes.items():
        keys = 4 * torch.randint(0, n_groups, (n,), device=dev, generator=g,
                                 dtype=torch.int64)
        cols = [keys, vals]
        runs = {v: [] for v, _ in variants}
        for i in range(WARMUP + REPEATS):
            for v, func in variants:       # alternate A, B, A, B, ...
                r = run_one(lib, cols, func, n_groups)
                if i >= WARMUP:
                    runs[v].append(r)
        a, b = runs["sum_i64n"], runs["sum_dec"]
        assert a[0][2:] == b[0][2:], \
            f"{name}: sum_i64n {a[0][2:]} vs sum_dec {b[0][2:]}"
        assert a[0][3] == int(vals.sum().item())
        line = {"shape": name, "rows": n, "groups": a[0][2],
                "warmup": WARMUP, "repeats": REPEATS}
        for v, rs in runs.items():
            line[v + "_wall_ms_min_med_max"] = spread([r[0] * 1e3 for r in rs])
            line[v + "_kernel_ms_min_med_max"] = spread([r[1] for r in rs])
        line["wall_ratio_dec_over_i64n"] = round(
            statistics.median(r[0] for r in b) /
            statistics.median(r[0] for r in a), 3)
        line["kernel_ratio_dec_over_i64n"] = round(
            statistics.median(r[1] for r in b) /
            statistics.median(r[1] for r in a), 3)
        print(json.dumps(line), flush=True)
        del keys, cols


if __name__ == "__main__":
    main()
