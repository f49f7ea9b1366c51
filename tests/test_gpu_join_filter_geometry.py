"""The join filter's geometry (GX_BLOOM_SHIFT, GX_BLOOM_K) never changes a
result.

The filter only gates the bucket read: a geometry may let more or fewer
non-matching rows through to the walk, but it must never drop a matching
row, so for every (shift, k) the emitted rows equal the CPU oracle's, with no
tolerance. Every reader of the filter is driven:
  k_probe_scan and k_probe      (gxop_join_probe_scan, then the composed
                                 scan + gxop_join_probe), INNER and SEMI;
  k_gj_probe_scan and k_gj_probe_inline
                                (gxop_groupjoin_probe_scan, then the composed
                                 scan + gxop_groupjoin_probe).
Builds of 1, 63, 64, 65 and 4,097 keys (twice each but the first) are forced
to carry a filter with GX_BLOOM=1: their shifted line count clamps at one
line, mask 0. The 70,000-key build takes the default gate. Half of the probe
keys are absent from the build and the probe key column carries NULLs.
"""
import numpy as np
import pytest

from galaxysql_amd import abi

from . import test_gpu_groupjoin_probe_scan as gj
from . import test_gpu_probe_scan as ps

pytestmark = pytest.mark.gpu

GEOMETRIES = [(s, k) for s in (0, 1, 3) for k in (1, 2, 3)]
SIZES = [1, 63, 64, 65, 4097, 70_000]
N_PROBE = 6000


def half_absent(raw, n_keys, rng):
    """Overwrite every other probe key with one no build holds (builds hold
    3i + 1); the rest keep their present keys. Returns raw."""
    key = raw[0][0]
    key[::2] = rng.integers(0, max(n_keys, 1), len(key[::2])) * 3 + 2
    return raw


def set_env(monkeypatch, shift, k, n_keys):
    if n_keys >= 65536:
        monkeypatch.delenv("GX_BLOOM", raising=False)   # the default gate
    else:
        monkeypatch.setenv("GX_BLOOM", "1")
    monkeypatch.setenv("GX_BLOOM_SHIFT", str(shift))
    monkeypatch.setenv("GX_BLOOM_K", str(k))


@pytest.mark.parametrize("n_keys", SIZES)
@pytest.mark.parametrize("shift,k", GEOMETRIES)
def test_plain_joins(shift, k, n_keys, monkeypatch):
    set_env(monkeypatch, shift, k, n_keys)
    rng = np.random.default_rng(1000 * n_keys + 10 * shift + k)
    dup = 1 if n_keys == 1 else 2
    build = ps.gen_build(rng, n_keys, dup=dup, with_nulls=n_keys > 1)
    raw = half_absent(ps.gen_raw(rng, N_PROBE, n_keys, "all", (0, 1)),
                      n_keys, rng)
    preds = [(1, abi.GT, ps.PRED_CUT["half"])]
    rows = ps.run_case(raw, build, preds, join_type=abi.INNER,
                       enable_bloom=True)
    assert rows > 0
    assert ps.run_case(raw, build, preds, join_type=abi.SEMI,
                       enable_bloom=True) > 0


@pytest.mark.parametrize("n_keys", SIZES)
@pytest.mark.parametrize("shift,k", GEOMETRIES)
def test_group_joins(shift, k, n_keys, monkeypatch):
    set_env(monkeypatch, shift, k, n_keys)
    rng = np.random.default_rng(2000 * n_keys + 10 * shift + k)
    dup = 1 if n_keys == 1 else 2
    build = gj.gen_build(rng, n_keys, dup=dup)
    raw = half_absent(gj.gen_raw(rng, N_PROBE, n_keys, match="all",
                                 null_cols=(0,)), n_keys, rng)
    got, _, ref, _, _, matched = gj.run_case(raw, build, gj.HALF)
    assert ref is not None and matched > 0
    # every present key occurs `dup` times in the build
    assert sum(c.n_rows for c in got) % dup == 0


def test_default_geometry(monkeypatch):
    """No geometry variable set: the rule of bloom_geometry, default gate."""
    for v in ("GX_BLOOM", "GX_BLOOM_SHIFT", "GX_BLOOM_K"):
        monkeypatch.delenv(v, raising=False)
    rng = np.random.default_rng(77)
    build = ps.gen_build(rng, 70_000, dup=2)
    raw = half_absent(ps.gen_raw(rng, N_PROBE, 70_000, "all", (0,)), 70_000,
                      rng)
    assert ps.run_case(raw, build, [(1, abi.GT, -1)], enable_bloom=True) > 0
