"""Sort / top-N operator timings (gxop_sort_*), one JSON line per shape.

Shapes (scale 1.0):
  q3_top10      12.9M rows x 6 columns (Q3's group count and result schema),
                ORDER BY F64 DESC, I32 ASC, K = 10
  q18_top100    the same rows, K = 100
  all_equal     12.9M rows whose first order column is one value, I32 second
                key, K = 10: the select's candidates are every row
  sort_12.9m    full sort of 12.9M rows on one I64 key (+ one I64 payload)
  sort_100m     full sort of 100M rows on one I64 key (+ one I64 payload)

Each top-N shape runs with GX_TOPN_SELECT=0 (full sort, then cut) and =1
(radix select, then sort of the candidates); the operator reads the variable
at create. Each variant: 2 warm-up runs, then 7 timed runs; the median wall
time and the median HIP-event time (stats()["kernel_ms"]) are printed. Wall
covers create, consume (a device-to-device append), build, the emitted
batch and close; inputs are device-resident, so there is no PCIe transfer.

Yardstick in the same job: torch.topk / torch.sort on the key column alone.
That does less (one key, no payload gather, no second key), so it is a floor,
not a bar to clear.

Run on an MI355X box:  python tools/bench_sort.py [scale]
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
from galaxysql_amd.chunk import I64, I32, F64
from galaxysql_amd.operators import SortExec

WARMUP, REPEATS = 2, 7
Q3_TYPES = [I64, I32, I32, F64, I64, I64]   # queries.Q3_RESULT_TYPES


def dev_chunk(cols, types):
    return [{"type": t, "values": c.data_ptr(), "n_rows": c.numel()}
            for c, t in zip(cols, types)]


def run_op(lib, cols, types, order, fetch, select):
    """-> (wall s, kernel ms, stats, first key of the result)."""
    if select is None:
        os.environ.pop("GX_TOPN_SELECT", None)
    else:
        os.environ["GX_TOPN_SELECT"] = str(select)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    # compact_rows past the input: time the one-shot ordering, not the
    # streaming compaction
    op = SortExec(lib, order, types, fetch=fetch, device=0,
                  expected_rows=cols[0].numel(),
                  compact_rows=cols[0].numel() + 1)
    keep = []
    gc = lib.to_gx_chunk(None, keep, device_ptrs=dev_chunk(cols, types))
    op.consume_raw(C.byref(gc))
    op.build_consume()
    out = C.POINTER(abi.GxResult)()
    lib.check(lib.lib.gxop_sort_next(op._op, C.byref(out)), "sort_next")
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    st = op.stats()
    rows = out.contents.chunk.n_rows
    lib.lib.gxop_result_release(out)
    op.close()
    os.environ.pop("GX_TOPN_SELECT", None)
    return wall, st["kernel_ms"], st, rows


def timed(fn):
    for _ in range(WARMUP):
        fn()
    ts = []
    for _ in range(REPEATS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3


def measure(lib, cols, types, order, fetch, select):
    for _ in range(WARMUP):
        run_op(lib, cols, types, order, fetch, select)
    runs = [run_op(lib, cols, types, order, fetch, select)
            for _ in range(REPEATS)]
    st = runs[0][2]
    return {"wall_ms": round(statistics.median(r[0] for r in runs) * 1e3, 3),
            "kernel_ms": round(statistics.median(r[1] for r in runs), 3),
            "used_select": st["used_select"],
            "select_passes": st["select_passes"],
            "candidates": st["candidates"], "rows_out": runs[0][3]}


def main():
    scale = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
    n = int(12_900_000 * scale)
    n_big = int(100_000_000 * scale)
    lib = abi.load_hip()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(3)

    def rnd(hi, count, dtype=torch.int64):
        return torch.randint(0, hi, (count,), device=dev, generator=g,
                             dtype=dtype)

    revenue = torch.rand(n, device=dev, generator=g,
                         dtype=torch.float64) * 5e5
    q3 = [rnd(1 << 40, n), rnd(1500, n, torch.int32) + 8000,
          torch.zeros(n, dtype=torch.int32, device=dev), revenue,
          rnd(1 << 40, n), rnd(8, n) + 1]
    q3_order = [(3, False), (1, True)]

    for name, cols, order, k in [
            ("q3_top10", q3, q3_order, 10),
            ("q18_top100", q3, q3_order, 100),
            # o_shippriority (column 2) is one value in Q3's result
            ("all_equal", q3, [(2, True), (1, True)], 10)]:
        res = {"shape": name, "rows": n, "cols": len(Q3_TYPES), "k": k,
               "warmup": WARMUP, "repeats": REPEATS}
        for select in (0, 1):
            res[f"select{select}"] = measure(lib, cols, Q3_TYPES, order, k,
                                             select)
        res["gate_default"] = measure(lib, cols, Q3_TYPES, order, k, None)
        key = cols[order[0][0]]
        res["torch_topk_key_only_ms"] = round(timed(
            lambda: torch.topk(key, k, largest=not order[0][1])), 3)
        res["wall_ratio_select_over_full"] = round(
            res["select1"]["wall_ms"] / res["select0"]["wall_ms"], 3)
        print(json.dumps(res), flush=True)
    del q3, revenue

    for name, rows in [("sort_12.9m", n), ("sort_100m", n_big)]:
        key = rnd(1 << 62, rows)
        pay = torch.arange(rows, device=dev, dtype=torch.int64)
        res = {"shape": name, "rows": rows, "cols": 2,
               "warmup": WARMUP, "repeats": REPEATS}
        res["full_sort"] = measure(lib, [key, pay], [I64, I64], [(0, True)],
                                   -1, None)
        res["torch_sort_key_only_ms"] = round(
            timed(lambda: torch.sort(key)), 3)
        res["rows_per_s"] = round(rows / (res["full_sort"]["wall_ms"] * 1e-3))
        print(json.dumps(res), flush=True)
        del key, pay
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
