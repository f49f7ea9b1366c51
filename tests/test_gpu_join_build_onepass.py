"""Single-pass inline-bucket join build against the CPU oracle.

The build hands out bucket ranks with one returning atomic per row, stores
ranks 0..3 inline and places later ranks through a spill list; with the
bloom on it also sets the key's two filter bits in the same pass. These
cases aim at exactly that: buckets that overflow (every key six times), one
bucket that takes thousands of spilled rows next to ordinary ones, a build
that is a single bucket, NULL build keys (never inserted), and a build
above the 65,536-row bloom gate — on the inline-I64-key path and on the
generic two-key path (row hash as entry key). Output rows are compared
exactly after sorting; probe and build payload columns carry row numbers,
so a misplaced entry shows up as a wrong position, not only a wrong
count."""
import numpy as np
import pytest

from galaxysql_amd import abi
from galaxysql_amd.chunk import I64, I32, chunks_from_columns
from galaxysql_amd.operators import EquiJoinKey, run_join

from .tabular import sorted_table

pytestmark = pytest.mark.gpu

HOT = 5_000            # rows sharing one key in the "hot" pattern
N_PROBE = 100_000
ABSENT_BASE = 1 << 40  # keys no build ever holds


@pytest.fixture(scope="module")
def libs():
    import os
    import subprocess
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run(["make", "-C", os.path.join(repo, "oracle")], check=True,
                   capture_output=True)
    return abi.load_oracle(), abi.load_hip()


def build_keys(pattern, n, rng):
    """-> (keys i64[n], nulls or None, distinct present keys, hot key or None)

    Key values are 1 mod 3 (the hot key is 2), so ABSENT_BASE + 3j never
    collides with them."""
    if pattern == "unique":
        k = rng.permutation(n).astype(np.int64) * 3 + 1
        return k, None, k, None
    if pattern == "six":
        d = np.arange((n + 5) // 6, dtype=np.int64) * 3 + 1
        k = rng.permutation(np.tile(d, 6)[:n])
        return k, None, d, None
    if pattern == "hot":
        # n unique keys plus one key HOT times
        u = np.arange(n, dtype=np.int64) * 3 + 1
        hot = np.int64(2)
        k = rng.permutation(np.concatenate([u, np.full(HOT, hot)]))
        return k, None, u, hot
    if pattern == "onekey":
        k = np.full(n, 7, dtype=np.int64)
        return k, None, k[:1], None
    if pattern == "nulls":
        k = rng.permutation(n).astype(np.int64) * 3 + 1
        nulls = (rng.random(n) < 0.10).astype(np.uint8)
        return k, nulls, k[nulls == 0], None
    raise AssertionError(pattern)


def second_key(k1):
    """I32 companion key of the two-key path, a function of the first"""
    return ((k1 * 7 + 3) % 1001).astype(np.int32)


CASES = [
    # (pattern, build rows, bloom, probe rows)
    ("unique", 5_000, False, N_PROBE),
    ("unique", 70_000, True, N_PROBE),
    ("six", 5_000, False, N_PROBE),
    ("six", 70_000, True, N_PROBE),
    ("hot", 5_000, False, N_PROBE),      # 5,000 unique + 5,000 hot rows
    ("hot", 70_000, True, N_PROBE),
    ("onekey", 5_000, False, 200),
    ("nulls", 5_000, False, N_PROBE),
    ("nulls", 70_000, True, N_PROBE),
]

_inputs = {}


def inputs(case, two_key):
    """Build and probe chunks of one case (made once, never modified)."""
    key = (case, two_key)
    if key in _inputs:
        return _inputs[key]
    pattern, n_build, _, n_probe = case
    rng = np.random.default_rng(1000 + CASES.index(case))
    bk, bnull, present, hot = build_keys(pattern, n_build, rng)
    nb = len(bk)
    # probe: half present keys, half absent ones; the hot key exactly 3x so
    # the output stays small
    half = n_probe // 2
    absent = ABSENT_BASE + 3 * rng.integers(0, 1 << 20, n_probe - half)
    if bnull is not None:
        # the values under NULL build keys must not match either: a build
        # that inserted those rows would show here
        dead = bk[bnull != 0]
        absent[:len(absent) // 2] = rng.choice(dead, len(absent) // 2)
    pk = np.concatenate([rng.choice(present, half), absent])
    if hot is not None:
        pk[:3] = hot
    pk = rng.permutation(pk).astype(np.int64)
    b_pay = np.arange(nb, dtype=np.int64)
    p_pay = np.arange(n_probe, dtype=np.int64)
    if not two_key:
        btypes, ptypes = [I64, I64], [I64, I64]
        bcols = [(bk, bnull), (b_pay, None)]
        pcols = [(pk, None), (p_pay, None)]
        keys = [EquiJoinKey(0, 0, I64)]
    else:
        btypes, ptypes = [I64, I32, I64], [I64, I32, I64]
        b2, p2 = second_key(bk), second_key(pk)
        # a tenth of the present probes agree on key 1 only
        flip = rng.random(n_probe) < 0.10
        p2 = np.where(flip, p2 + 1, p2).astype(np.int32)
        b2null = None
        if bnull is not None:   # NULLs in either key column
            b2null = (rng.random(nb) < 0.05).astype(np.uint8)
        bcols = [(bk, bnull), (b2, b2null), (b_pay, None)]
        pcols = [(pk, None), (p2, None), (p_pay, None)]
        keys = [EquiJoinKey(0, 0, I64), EquiJoinKey(1, 1, I32)]
    build = chunks_from_columns(btypes, bcols, chunk_size=16_384)
    probe = chunks_from_columns(ptypes, pcols, chunk_size=N_PROBE)
    _inputs[key] = (build, probe, ptypes, btypes, keys)
    return _inputs[key]


JOINS = [abi.INNER, abi.LEFT, abi.SEMI, abi.ANTI]


@pytest.mark.parametrize("two_key", [False, True], ids=["i64", "i64_i32"])
@pytest.mark.parametrize("join_type", JOINS,
                         ids=["inner", "left", "semi", "anti"])
@pytest.mark.parametrize("case", CASES,
                         ids=[f"{c[0]}{c[1]}" for c in CASES])
def test_onepass_build_matches_oracle(libs, case, join_type, two_key):
    oracle, hip = libs
    build, probe, ptypes, btypes, keys = inputs(case, two_key)
    ref = run_join(oracle, join_type, keys, build, probe, ptypes, btypes,
                   device=-1)
    got = run_join(hip, join_type, keys, build, probe, ptypes, btypes,
                   device=0, enable_bloom=case[2])
    n_cols = len(ptypes) + (len(btypes)
                            if join_type in (abi.INNER, abi.LEFT) else 0)
    r, g = sorted_table(ref, n_cols), sorted_table(got, n_cols)
    assert r.shape == g.shape
    assert np.array_equal(r, g)
    if join_type == abi.INNER and case[0] != "nulls":
        assert len(g) > 0
