"""DISTINCT aggregates, the parts that need no GPU: the ABI constants, the two
expected-result references (tests/distinct_ref.py) checked against each
other and against the DistinctSetTest golden vectors, the oracle's loud
rejection, and the host-side planning helpers."""
import os
import re
import subprocess

import numpy as np
import pytest

from galaxysql_amd import abi
from galaxysql_amd.chunk import (I64, I32, F64, SLICE, chunks_from_columns,
                                 multiset)
from galaxysql_amd.exchange import final_agg_specs
from galaxysql_amd.operators import HashAggExec

from . import distinct_ref as dr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = {"GX_AGG_COUNT_DISTINCT": (abi.COUNT_DISTINCT, 23),
         "GX_AGG_SUM_I64_DISTINCT": (abi.SUM_I64_DISTINCT, 24),
         "GX_AGG_SUM_I64N_DISTINCT": (abi.SUM_I64N_DISTINCT, 25),
         "GX_AGG_SUM_F64_DISTINCT": (abi.SUM_F64_DISTINCT, 26),
         "GX_AGG_AVG_F64_DISTINCT": (abi.AVG_F64_DISTINCT, 27)}


@pytest.fixture(scope="module")
def oracle():
    subprocess.run(["make", "-C", os.path.join(REPO, "oracle")], check=True,
                   capture_output=True)
    return abi.load_oracle()


def test_constants_match_header():
    with open(os.path.join(REPO, "include", "gxop.h")) as f:
        text = f.read()
    parsed = {m.group(1): int(m.group(2))
              for m in re.finditer(r"\b(GX_AGG_\w+)\s*=\s*(\d+)", text)}
    for name, (const, value) in NAMES.items():
        assert parsed[name] == value == const, name
    assert abi.DISTINCT_FUNCS == {c for c, _ in NAMES.values()}
    # the new values extend the enum without touching the old ones
    assert parsed["GX_AGG_SUM_I64N"] == abi.SUM_I64N == 22
    assert parsed["GX_AGG_COUNT_ROW"] == abi.COUNT_ROW == 0


def test_golden_replay_and_references(oracle):
    gold = dr.load_golden()
    # replaying the chunks through a literal set reproduces the recorded
    # first-seen flags of DistinctSet.checkDistinct
    seen = set()
    for ch in gold["chunks"]:
        flags = []
        for pair in zip(ch["gids"], ch["values"]):
            flags.append(pair not in seen)
            seen.add(pair)
        assert flags == ch["first_seen"]
    chunks = dr.golden_chunks(gold)
    aggs = [(abi.COUNT_DISTINCT, 1)]
    exp = multiset(dr.golden_expected_rows(gold))
    assert multiset(dr.brute_agg([0], aggs, chunks)) == exp
    assert multiset(dr.rewrite_agg(oracle, [0], aggs, [I64, SLICE],
                                   chunks)) == exp


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_references_agree_on_random_inputs(oracle, seed):
    rng = np.random.default_rng(seed)
    n = 4000
    gk = rng.integers(0, 150, n, dtype=np.int64)
    types = [I64, I64, F64, I32]
    chunks = chunks_from_columns(types, [
        (gk, (rng.random(n) < 0.03).astype(np.uint8)),
        (gk * 7 + rng.integers(0, 12, n), (rng.random(n) < 0.1).astype(np.uint8)),
        (rng.integers(-8, 8, n).astype(np.float64),
         (rng.random(n) < 0.1).astype(np.uint8)),
        (rng.integers(-5, 5, n, dtype=np.int32), None)], chunk_size=700)
    aggs = [(abi.COUNT_ROW, -1), (abi.COUNT_DISTINCT, 1),
            (abi.SUM_I64_DISTINCT, 1), (abi.SUM_I64N_DISTINCT, 3),
            (abi.SUM_F64_DISTINCT, 2), (abi.AVG_F64_DISTINCT, 2),
            (abi.COUNT_DISTINCT, 2), (abi.SUM_I64, 1), (abi.MIN_I64, 1)]
    for group_cols in ([0], []):
        a = dr.brute_agg(group_cols, aggs, chunks)
        b = dr.rewrite_agg(oracle, group_cols, aggs, types, chunks)
        assert len(a) == len(b)
        assert multiset(a, f64_round=9) == multiset(b, f64_round=9)


def test_references_agree_on_empty_global(oracle):
    aggs = [(abi.COUNT_DISTINCT, 0), (abi.SUM_I64_DISTINCT, 0),
            (abi.SUM_I64N_DISTINCT, 0), (abi.SUM_F64_DISTINCT, 0),
            (abi.AVG_F64_DISTINCT, 0)]
    exp = [(0, 0, None, None, None)]
    assert dr.brute_agg([], aggs, []) == exp
    assert dr.rewrite_agg(oracle, [], aggs, [I64], []) == exp


@pytest.mark.parametrize("name", sorted(NAMES))
def test_oracle_rejects_distinct(oracle, name):
    """The checker library does not know DISTINCT and says so, instead of
    computing the plain aggregate."""
    with pytest.raises(RuntimeError) as e:
        HashAggExec(oracle, [0], [(NAMES[name][0], 1)], [I64, I64], device=-1)
    assert str(e.value).split("gxop_agg_create:", 1)[1].strip()


@pytest.mark.parametrize("name", sorted(NAMES))
def test_final_agg_specs_refuses_distinct(name):
    with pytest.raises(ValueError) as e:
        final_agg_specs(1, [(abi.COUNT_ROW, -1), (NAMES[name][0], 1)])
    msg = str(e.value)
    assert "DISTINCT" in msg
    assert "huffle" in msg and "group keys" in msg and "single phase" in msg


def test_distinct_of():
    assert abi.distinct_of(abi.COUNT_COL) == abi.COUNT_DISTINCT
    assert abi.distinct_of(abi.SUM_I64) == abi.SUM_I64_DISTINCT
    assert abi.distinct_of(abi.SUM_I64N) == abi.SUM_I64N_DISTINCT
    assert abi.distinct_of(abi.SUM_F64) == abi.SUM_F64_DISTINCT
    assert abi.distinct_of(abi.AVG_F64) == abi.AVG_F64_DISTINCT
    for f in (abi.MIN_I64, abi.MAX_I64, abi.MIN_F64, abi.MAX_F64,
              abi.BIT_AND, abi.BIT_OR, abi.BIT_XOR):
        assert abi.distinct_of(f) == f
    for f in (abi.COUNT_ROW, abi.RANK, abi.DENSE_RANK, abi.FIRST_VALUE,
              abi.NTILE, abi.PERCENT_RANK, abi.COUNT_DISTINCT, 99):
        with pytest.raises(ValueError):
            abi.distinct_of(f)
