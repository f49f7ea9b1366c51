"""Slot-indexed fused accumulate for per-group records of up to 4 u64.

Records of 3 and 4 u64 now live beside their hash slot and are updated in
the insert kernel; a 6-u64 record must still take the gid-indexed two-pass
path. Each case is checked against the CPU oracle and against the same
library run with GX_AGG_SLOT_STRIDE=2 (the old gate: everything here wider
than 2 goes by gid). f64 inputs are multiples of 0.25 below 2^20, so every
sum is exact in any order and all columns compare with ==.

Shapes: one 300,000-row chunk with expected_groups=0 (above the 2^18
large-chunk threshold; the 2048-slot start forces several x4 rehashes that
migrate records and rerun only the failed rows), the same rows in seven
chunks, and 1,000-row chunks (inline-gid mode)."""
import numpy as np
import pytest

from galaxysql_amd import abi
from galaxysql_amd.chunk import I64, I32, F64, chunks_from_columns
from galaxysql_amd.operators import run_agg

from .tabular import sorted_table

pytestmark = pytest.mark.gpu

N_ROWS = 300_000
N_GROUPS = 100_000

# input columns: 0..2 keys (I64, I32, I32), 3 f64 value, 4 i64 value
TYPES = [I64, I32, I32, F64, I64]

AGG_SETS = {
    "sumf_sumi_count": [(abi.SUM_F64, 3), (abi.SUM_I64, 4),
                        (abi.COUNT_ROW, -1)],               # 4 u64 (Q3's)
    "avg_countcol": [(abi.AVG_F64, 3), (abi.COUNT_COL, 4)],  # 3
    "min_sumi": [(abi.MIN_I64, 4), (abi.SUM_I64, 4)],        # 3
    "sumf_x3": [(abi.SUM_F64, 3)] * 3,                       # 6: gid path
}
KEY_SETS = {"k3": [0, 1, 2], "k1": [0]}
SHAPES = {"one_chunk": N_ROWS, "seven_chunks": (N_ROWS + 6) // 7,
          "chunks_1000": 1_000}


@pytest.fixture(scope="module")
def libs():
    import os
    import subprocess
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run(["make", "-C", os.path.join(repo, "oracle")], check=True,
                   capture_output=True)
    return abi.load_oracle(), abi.load_hip()


_columns = {}


def columns(null_keys):
    """The 300,000 input rows (made once): 100,000 distinct key triples,
    20 % NULL values, optionally ~3 % NULLs per key column."""
    if null_keys in _columns:
        return _columns[null_keys]
    rng = np.random.default_rng(2024)
    # every group at least once, the rest at random
    g = rng.permutation(np.concatenate(
        [np.arange(N_GROUPS), rng.integers(0, N_GROUPS, N_ROWS - N_GROUPS)]))
    gk0 = rng.permutation(N_GROUPS).astype(np.int64) * 5 + (1 << 33)
    gk1 = rng.integers(-50, 50, N_GROUPS).astype(np.int32)
    gk2 = rng.integers(0, 3, N_GROUPS).astype(np.int32)
    f = rng.integers(0, 1 << 22, N_ROWS).astype(np.float64) * 0.25
    i = rng.integers(-(1 << 40), 1 << 40, N_ROWS).astype(np.int64)
    fn = (rng.random(N_ROWS) < 0.20).astype(np.uint8)
    inn = (rng.random(N_ROWS) < 0.20).astype(np.uint8)
    kn = [None, None, None]
    if null_keys:
        kn = [(rng.random(N_ROWS) < 0.03).astype(np.uint8) for _ in range(3)]
    _columns[null_keys] = [(gk0[g], kn[0]), (gk1[g], kn[1]), (gk2[g], kn[2]),
                           (f, fn), (i, inn)]
    return _columns[null_keys]


_refs = {}


def oracle_table(oracle, aggs, keys, null_keys):
    key = (aggs, keys, null_keys)
    if key not in _refs:
        chunks = chunks_from_columns(TYPES, columns(null_keys),
                                     chunk_size=N_ROWS)
        out = run_agg(oracle, KEY_SETS[keys], AGG_SETS[aggs], TYPES, chunks,
                      device=-1)
        _refs[key] = sorted_table(out, len(KEY_SETS[keys]) +
                                  len(AGG_SETS[aggs]))
    return _refs[key]


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("null_keys", [False, True],
                         ids=["keys_notnull", "keys_null"])
@pytest.mark.parametrize("keys", list(KEY_SETS))
@pytest.mark.parametrize("aggs", list(AGG_SETS))
def test_wide_slot_matches_oracle_and_gid_path(libs, monkeypatch, aggs, keys,
                                               null_keys, shape):
    oracle, hip = libs
    n_cols = len(KEY_SETS[keys]) + len(AGG_SETS[aggs])
    chunks = chunks_from_columns(TYPES, columns(null_keys),
                                 chunk_size=SHAPES[shape])

    def run_hip():
        return sorted_table(
            run_agg(hip, KEY_SETS[keys], AGG_SETS[aggs], TYPES, chunks,
                    expected_groups=0, device=0), n_cols)

    monkeypatch.delenv("GX_AGG_SLOT_STRIDE", raising=False)
    got = run_hip()
    ref = oracle_table(oracle, aggs, keys, null_keys)
    assert got.shape == ref.shape
    assert np.array_equal(got, ref)
    if not null_keys:
        assert len(got) == N_GROUPS

    monkeypatch.setenv("GX_AGG_SLOT_STRIDE", "2")
    old_gate = run_hip()
    assert np.array_equal(old_gate, got)
