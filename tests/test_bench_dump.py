"""bench.py --dump-outputs: the canonical row image is independent of the
order an operator emitted its rows in (CPU), and a plain small-scale run
writes self-consistent float64 outputs of the last timed step and skips
the --full-only CPU baseline (gpu)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_canonical_rows_order_independent():
    import torch
    import bench
    g = torch.Generator().manual_seed(7)
    n = 20_000
    key = 4 * torch.randperm(n, generator=g)
    val = torch.rand(n, generator=g, dtype=torch.float64)
    perm = torch.randperm(n, generator=g)
    a = bench.canonical_rows([key, val], [0], max_rows=1000)
    b = bench.canonical_rows([key[perm], val[perm]], [0], max_rows=1000)
    assert a.dtype == np.float64 and a.shape[1] == 2
    assert 0 < a.shape[0] <= 1000
    assert np.array_equal(a, b)
    assert np.all(np.diff(a[:, 0]) > 0)
    # under the cap nothing is dropped
    full = bench.canonical_rows([key, val], [0], max_rows=n)
    assert full.shape == (n, 2)
    assert np.array_equal(full[:, 0], np.arange(n) * 4.0)


@pytest.mark.gpu
def test_plain_run_dumps_last_step(tmp_path):
    out = subprocess.run(
        [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
         "--steps", "2", "--warmup", "1", "--c3-scale", "0.002",
         "--dump-outputs", str(tmp_path)],
        capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["steps"] == 2 and res["ms_per_step"] > 0
    assert res["cpu_baseline"] is None  # the baseline runs only with --full

    files = sorted(os.listdir(tmp_path))
    assert files == ["counts.npy", "group_totals.npy", "groups.npy"]
    arrs = {f[:-4]: np.load(tmp_path / f) for f in files}
    assert all(a.dtype == np.float64 for a in arrs.values())
    assert sum(a.nbytes for a in arrs.values()) <= 64 << 20

    counts, totals, groups = (arrs["counts"], arrs["group_totals"],
                              arrs["groups"])
    joined, n_groups = counts[4], counts[5]
    assert n_groups == res["config"]["groups_last_step"] > 0
    # this scale is under the sampling cap: every group is written
    assert groups.shape == (int(n_groups), 6) and totals[0] == n_groups
    assert np.all(np.diff(groups[:, 0]) > 0)          # sorted, unique key
    assert groups[:, 5].sum() == joined == totals[3]  # COUNT(*) covers join
    assert groups[:, 4].sum() == totals[2]            # exact scaled-int sum
    # SUM(revenue) f64 vs the exact scale-4 integer sum: the project's
    # rel-tol for f64 aggregates
    assert np.allclose(groups[:, 3] * 1e4, groups[:, 4], rtol=1e-9, atol=0)
