"""A/B: low-cardinality GROUP BY. The hash aggregation's block-local (LDS)
accumulate pass against GX_AGG_LOCAL=0 (a global atomic per row and
aggregate on the few group records) in the same build, one device, data
device-resident.

Legs (python tools/bench_lowcard.py LEG):
  q1shape    4 groups on two I32 codes, Q1's 8 aggregates (22-u64 record).
             A/B from 2^22 rows, x4 while the =0 leg stays under
             OFF_LIMIT_S; then the local path alone at LARGE_ROWS
  global     SUM_I64 + COUNT(*) without GROUP BY, same plan
  replicas   q1shape and global, the local path alone at REPL_ROWS rows with
             the replica count capped (GX_AGG_LOCAL_REPLICAS = 1, 4, 16,
             unset)
  sweep      group count 1..1024 at SWEEP_ROWS rows in one chunk: a narrow
             record (COUNT + SUM_I64, hint = the count: =0 is the slot-fused
             insert) and Q1's wide record (as far as it fits the LDS budget)
  crossover  CROSS_ROWS rows fed in chunks of 2^12..2^20 rows, 4 groups,
             GX_AGG_LOCAL=1 against =0, narrow and wide record
  capsweep   CROSS_ROWS rows in chunks of 2^16 and 2^18 rows, 16..1024 groups,
             GX_AGG_LOCAL=1 against =0: the cap at the gate's chunk sizes
  q1chain    queries.run_q1 end to end over CHAIN_ROWS device-resident rows
  all        every leg, each in a fresh child process under its own timeout;
             stops at the first leg that fails or runs out of time

A group count above the library's cap (local_groups_cap) runs the plain
path in both variants: its line then shows local_rows = 0.

The two variants of a shape run ALTERNATELY, WARMUP warm-up runs each, then
REPEATS timed runs each; min / median / max of the op's HIP-event time
(stats()["kernel_ms"]: insert, gid assignment and accumulate of every
consume) and of wall time (create to emitted result). One JSON line per
measurement. GX_AGG_LOCAL is read at op create, so one process sets it per
run. Results of the two variants are compared (same groups, same COUNT and
integer sums).

Run on an MI355X box, each leg under `timeout`:
    timeout -k 10 300 python tools/bench_lowcard.py q1shape
"""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from galaxysql_amd import abi, queries
from galaxysql_amd.chunk import I32, I64
from galaxysql_amd.operators import HashAggExec

WARMUP, REPEATS = 1, 5
OFF_LIMIT_S = 1.0          # grow the A/B only while the =0 leg is below this
MAX_AB_ROWS = 1 << 26
LARGE_ROWS = 1 << 27
SWEEP_ROWS = 1 << 23
CROSS_ROWS = 1 << 22
REPL_ROWS = 1 << 26
CHAIN_ROWS = 1 << 27
LEG_TIMEOUT_S = {"q1shape": 240, "global": 180, "replicas": 120,
                 "sweep": 300, "crossover": 240, "capsweep": 240, "q1chain": 180}

WIDE_TYPES = queries.Q1_SCAN_TYPES          # flag, status, 5 x I64
NARROW_TYPES = [I64, I64]
NARROW_AGGS = [(abi.COUNT_ROW, -1), (abi.SUM_I64, 1)]
GLOBAL_AGGS = [(abi.SUM_I64, 1), (abi.COUNT_ROW, -1)]


def set_local(v):
    if v is None:
        os.environ.pop("GX_AGG_LOCAL", None)
    else:
        os.environ["GX_AGG_LOCAL"] = v


def dev_chunk(lib, cols, types, keep, a=0, b=None):
    b = cols[0].numel() if b is None else b
    return lib.to_gx_chunk(None, keep, device_ptrs=[
        {"type": t, "values": c[a:b].data_ptr(), "n_rows": b - a}
        for c, t in zip(cols, types)])


def run_one(lib, group_cols, aggs, types, cols, hint, chunk_rows=None,
            count_col=None):
    """One op over the columns. Returns (wall s, kernel ms, local_rows,
    replicas, groups, total of result column count_col)."""
    n = cols[0].numel()
    step = chunk_rows or n
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    op = HashAggExec(lib, group_cols, aggs, types, expected_groups=hint,
                     device=0)
    try:
        for a in range(0, n, step):
            keep = []
            gc = dev_chunk(lib, cols, types, keep, a, min(a + step, n))
            lib.check(lib.lib.gxop_agg_consume(op._op, C.byref(gc)),
                      "agg_consume")
        op.build_consume()
        out = C.POINTER(abi.GxResult)()
        lib.check(lib.lib.gxop_agg_next(op._op, C.byref(out)), "agg_next")
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        groups = out.contents.chunk.n_rows
        total = None
        if count_col is not None:
            s = torch.empty(groups, dtype=torch.int64, device=cols[0].device)
            lib.check(lib.lib.gxop_result_copy_col(
                out, count_col, C.c_void_p(s.data_ptr()), None), "copy_col")
            total = int(s.sum().item())
        lib.lib.gxop_result_release(out)
        ls = op.local_stats()
        return (wall, op.stats()["kernel_ms"], ls["local_rows"],
                ls["replicas"], groups, total)
    finally:
        op.close()


def spread(xs):
    return [round(min(xs), 3), round(statistics.median(xs), 3),
            round(max(xs), 3)]


def ab(lib, name, group_cols, aggs, types, cols, hint, count_col,
       on=None, off="0", chunk_rows=None, extra=None):
    """Alternate off / on; one JSON line. Returns the =0 leg's median wall
    seconds."""
    n = cols[0].numel()
    runs = {"off": [], "on": []}
    for i in range(WARMUP + REPEATS):
        for v, env in (("off", off), ("on", on)):
            set_local(env)
            r = run_one(lib, group_cols, aggs, types, cols, hint,
                        chunk_rows, count_col)
            if i >= WARMUP:
                runs[v].append(r)
    set_local(None)
    a, b = runs["off"], runs["on"]
    assert a[0][4:] == b[0][4:], f"{name}: off {a[0][4:]} vs on {b[0][4:]}"
    assert a[0][2] == 0, "GX_AGG_LOCAL=0 went local"
    line = {"leg": name, "rows": n, "groups": a[0][4],
            "chunk_rows": chunk_rows or n, "warmup": WARMUP,
            "repeats": REPEATS, "local_rows": b[0][2], "replicas": b[0][3]}
    line.update(extra or {})
    for v, rs in runs.items():
        line[v + "_kernel_ms_min_med_max"] = spread([r[1] for r in rs])
        line[v + "_wall_ms_min_med_max"] = spread([r[0] * 1e3 for r in rs])
    mo = statistics.median(r[1] for r in a)
    ml = statistics.median(r[1] for r in b)
    line["kernel_speedup_on_over_off"] = round(mo / ml, 2)
    line["on_rows_per_s"] = round(n / (ml * 1e-3) / 1e9, 3)   # G rows/s
    print(json.dumps(line), flush=True)
    return statistics.median(r[0] for r in a)


def local_only(lib, name, group_cols, aggs, types, cols, hint, count_col):
    set_local(None)
    rs = [run_one(lib, group_cols, aggs, types, cols, hint, None, count_col)
          for _ in range(WARMUP + REPEATS)][WARMUP:]
    n = cols[0].numel()
    assert rs[0][2] == n, "the large-N leg did not go local"
    ml = statistics.median(r[1] for r in rs)
    print(json.dumps({
        "leg": name, "rows": n, "groups": rs[0][4], "local_rows": rs[0][2],
        "replicas": rs[0][3],
        "on_kernel_ms_min_med_max": spread([r[1] for r in rs]),
        "on_wall_ms_min_med_max": spread([r[0] * 1e3 for r in rs]),
        "on_rows_per_s": round(n / (ml * 1e-3) / 1e9, 3),
        "input_GBps": round(n * row_bytes(types, aggs, bool(group_cols)) /
                            (ml * 1e-3) / 1e9, 1)}), flush=True)


def row_bytes(types, aggs, grouped):
    """Input bytes the accumulate pass reads per row: the values and, when
    grouped, the 4-B slot index."""
    used = {c for _, c in aggs if c >= 0}
    return sum(4 if types[c] == I32 else 8 for c in used) + (4 if grouped
                                                              else 0)


def wide_cols(n, n_groups, g):
    """Q1's projected chunk: two I32 codes spanning n_groups groups + five
    I64 measures in the ranges of qty, price, disc_price, charge, disc."""
    dev = torch.device("cuda:0")
    gid = torch.randint(0, n_groups, (n,), device=dev, generator=g,
                        dtype=torch.int32)
    cols = [gid // 2, gid % 2]
    for hi in (5001, 10_500_000, 1_050_000_000, 113_400_000_000, 11):
        cols.append(torch.randint(1, hi, (n,), device=dev, generator=g,
                                  dtype=torch.int64))
    return cols


def narrow_cols(n, n_groups, g):
    dev = torch.device("cuda:0")
    return [torch.randint(0, n_groups, (n,), device=dev, generator=g,
                          dtype=torch.int64) * 4,
            torch.randint(1, 10_000_000, (n,), device=dev, generator=g,
                          dtype=torch.int64)]


def gen():
    return torch.Generator(device=torch.device("cuda:0")).manual_seed(31)


def leg_grow(lib, name, make_cols, group_cols, aggs, types, hint, count_col):
    g = gen()
    n = 1 << 22
    while True:
        cols = make_cols(n, g)
        off_s = ab(lib, name, group_cols, aggs, types, cols, hint, count_col)
        del cols
        if off_s >= OFF_LIMIT_S or n >= MAX_AB_ROWS:
            break
        n *= 4
    cols = make_cols(LARGE_ROWS, g)
    local_only(lib, name + "_large", group_cols, aggs, types, cols, hint,
               count_col)


def leg_q1shape(lib):
    leg_grow(lib, "q1shape", lambda n, g: wide_cols(n, 4, g), [0, 1],
             queries.q1_aggs(), WIDE_TYPES, 6, 9)


def leg_global(lib):
    leg_grow(lib, "global", lambda n, g: narrow_cols(n, 1, g), [],
             GLOBAL_AGGS, NARROW_TYPES, 0, 1)


def leg_replicas(lib):
    """The local path alone, replica count capped: same-address LDS atomics
    only show once the kernel is not launch-bound, so at REPL_ROWS rows."""
    g = gen()
    wide, nar = wide_cols(REPL_ROWS, 4, g), narrow_cols(REPL_ROWS, 1, g)
    for rep in ("1", "4", "16", None):
        if rep is None:
            os.environ.pop("GX_AGG_LOCAL_REPLICAS", None)
        else:
            os.environ["GX_AGG_LOCAL_REPLICAS"] = rep
        local_only(lib, f"replicas_q1shape_cap{rep}", [0, 1],
                   queries.q1_aggs(), WIDE_TYPES, wide, 6, 9)
        local_only(lib, f"replicas_global_cap{rep}", [], GLOBAL_AGGS,
                   NARROW_TYPES, nar, 0, 1)
    os.environ.pop("GX_AGG_LOCAL_REPLICAS", None)


def leg_sweep(lib):
    g = gen()
    probe = HashAggExec(lib, [0, 1], queries.q1_aggs(), WIDE_TYPES, device=0)
    wide_cap = probe.local_stats()["local_groups_cap"]
    probe.close()
    k = 1
    while k <= 1024:
        cols = narrow_cols(SWEEP_ROWS, k, g)
        ab(lib, "sweep_narrow", [0], NARROW_AGGS, NARROW_TYPES, cols, k, 1,
           on="1")
        del cols
        if k <= wide_cap:
            cols = wide_cols(SWEEP_ROWS, k, g)
            ab(lib, "sweep_wide", [0, 1], queries.q1_aggs(), WIDE_TYPES,
               cols, k, 9, on="1")
            del cols
        k *= 2


def leg_crossover(lib):
    g = gen()
    wide, nar = wide_cols(CROSS_ROWS, 4, g), narrow_cols(CROSS_ROWS, 4, g)
    for sh in range(12, 21, 2):
        ab(lib, "crossover_wide", [0, 1], queries.q1_aggs(), WIDE_TYPES,
           wide, 6, 9, on="1", chunk_rows=1 << sh)
        ab(lib, "crossover_narrow", [0], NARROW_AGGS, NARROW_TYPES, nar, 4,
           1, on="1", chunk_rows=1 << sh)


def leg_capsweep(lib):
    """The group-count sweep again at the chunk sizes next to the gate: the
    flush is touched groups x stride atomics per block, so many groups in a
    small chunk are the local path's worst case."""
    g = gen()
    probe = HashAggExec(lib, [0, 1], queries.q1_aggs(), WIDE_TYPES, device=0)
    wide_cap = probe.local_stats()["local_groups_cap"]
    probe.close()
    for sh in (16, 18):
        for k in (16, 64, 128, 256, 512, 1024):
            cols = narrow_cols(CROSS_ROWS, k, g)
            ab(lib, "capsweep_narrow", [0], NARROW_AGGS, NARROW_TYPES, cols,
               k, 1, on="1", chunk_rows=1 << sh)
            del cols
            if k <= wide_cap:
                cols = wide_cols(CROSS_ROWS, k, g)
                ab(lib, "capsweep_wide", [0, 1], queries.q1_aggs(),
                   WIDE_TYPES, cols, k, 9, on="1", chunk_rows=1 << sh)
                del cols


def leg_q1chain(lib):
    dev = torch.device("cuda:0")
    g = gen()
    n = CHAIN_ROWS
    ship = torch.randint(8036, 10562, (n,), device=dev, generator=g,
                         dtype=torch.int32)
    late = ship > 9298
    status = late.to(torch.int32)
    flag = torch.where(late, 1, 2 * torch.randint(
        0, 2, (n,), device=dev, generator=g, dtype=torch.int32)).to(
            torch.int32)
    raw = [flag, status, ship,
           torch.randint(1, 51, (n,), device=dev, generator=g,
                         dtype=torch.int64) * 100,
           torch.randint(90_000, 10_500_000, (n,), device=dev, generator=g,
                         dtype=torch.int64),
           torch.randint(0, 11, (n,), device=dev, generator=g,
                         dtype=torch.int64),
           torch.randint(0, 9, (n,), device=dev, generator=g,
                         dtype=torch.int64)]
    set_local(None)
    walls, infos = [], []
    for i in range(WARMUP + REPEATS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        chunks, info = queries.run_q1(lib, 0, raw, chunk_rows=1 << 24)
        torch.cuda.synchronize()
        if i >= WARMUP:
            walls.append(time.perf_counter() - t0)
            infos.append(info)
    kept = infos[0]["lineitem_kept"]
    assert sum(c.n_rows for c in chunks) == 3
    assert infos[0]["local_rows"] == kept
    # bytes the chain moves at least: the raw columns once (44 B/row), the
    # projected chunk written by the scan and read by the aggregation
    # (2 x 48 B per kept row), and the aggregation's per-row hash and slot
    # index, written and read once each (16 B per kept row)
    moved = n * 44 + kept * (2 * 48 + 16)
    med = statistics.median(walls)
    print(json.dumps({
        "leg": "q1chain", "rows": n, "kept": kept, "chunk_rows": 1 << 24,
        "wall_ms_min_med_max": spread([w * 1e3 for w in walls]),
        "agg_kernel_ms_min_med_max": spread(
            [i["agg_kernel_ms"] for i in infos]),
        "bytes_moved_GB": round(moved / 1e9, 2),
        "GBps": round(moved / med / 1e9, 1),
        "hbm_fraction_of_8TBps": round(moved / med / 8e12, 3)}), flush=True)


LEGS = {"q1shape": leg_q1shape, "global": leg_global,
        "replicas": leg_replicas, "sweep": leg_sweep,
        "crossover": leg_crossover, "capsweep": leg_capsweep,
        "q1chain": leg_q1chain}


def main():
    leg = sys.argv[1] if len(sys.argv) > 1 else "all"
    if leg == "all":
        for name in LEGS:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__),
                                 name], timeout=LEG_TIMEOUT_S[name]).returncode
            if rc != 0:
                sys.exit(f"leg {name} failed (exit {rc}): stopping")
        return
    LEGS[leg](abi.load_hip())


if __name__ == "__main__":
    main()
