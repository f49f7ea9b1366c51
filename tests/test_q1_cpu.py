"""Q1's host side: the generator, the Python-integer reference against a
brute-force row loop, and the ABI constants the chain relies on."""
import ctypes as C

import numpy as np

from galaxysql_amd import abi, queries
from galaxysql_amd.chunk import I32, I64


def brute_q1(cols, cutoff):
    """Row-at-a-time Q1, nothing shared with ref_q1_numpy but the rounding
    rule (half-up on the magnitude at scale 4)."""
    def val(c, i):
        return None if (c[1] is not None and c[1][i]) else int(c[0][i])

    groups = {}
    for i in range(len(cols[0][0])):
        f, s, ship, q, p, d, t = (val(c, i) for c in cols)
        if ship is None or ship > cutoff:
            continue
        g = groups.setdefault((f, s), {"n": 0, "sum": [0] * 5, "cnt": [0] * 5})
        g["n"] += 1
        dp = None if p is None or d is None else p * (100 - d)
        ch = None if dp is None or t is None else dp * (100 + t)
        for k, v in enumerate((q, p, dp, ch, d)):
            if v is not None:
                g["sum"][k] += v
                g["cnt"][k] += 1
    rows = []
    for (f, s) in sorted(groups):
        g = groups[(f, s)]

        def total(k, scale):
            return (g["sum"][k], scale) if g["cnt"][k] else None

        def avg(k):
            if not g["cnt"][k]:
                return None
            tot, cnt = g["sum"][k], g["cnt"][k]
            q2, r = divmod(abs(tot) * 100, cnt)   # scale 2 -> scale 4
            q2 += 1 if 2 * r >= cnt else 0
            return (-q2 if tot < 0 else q2, 4)

        rows.append((f, s, total(0, 2), total(1, 2), total(2, 4),
                     total(3, 6), avg(0), avg(1), avg(4), g["n"]))
    return rows


def test_ref_q1_matches_brute_force():
    for nulls in (False, True):
        cols = queries.gen_q1_numpy(np.random.default_rng(4201), 2000,
                                    nulls=nulls)
        want = brute_q1(cols, queries.Q1_CUTOFF_DAYS)
        assert queries.ref_q1_numpy(cols) == want
        assert 3 <= len(want) <= 4
        assert sum(r[-1] for r in want) < 2000      # the filter drops rows


def test_ref_q1_all_null_group():
    """A group whose measures are all NULL gives NULL sums and averages."""
    cols = queries.gen_q1_numpy(np.random.default_rng(4202), 500, nulls=True)
    cols = [(v, None if nl is None else nl.copy()) for v, nl in cols]
    for c in (3, 4, 5, 6):
        cols[c][1][cols[0][0] == 2] = 1
    rows = queries.ref_q1_numpy(cols)
    assert rows == brute_q1(cols, queries.Q1_CUTOFF_DAYS)
    r = [r for r in rows if r[0] == 2][0]
    assert r[2:9] == (None,) * 7 and r[9] > 0


def test_gen_q1_shape_and_dtypes():
    n = 5000
    cols = queries.gen_q1_numpy(np.random.default_rng(4203), n)
    assert len(cols) == len(queries.Q1_LINEITEM_TYPES) == 7
    want_dt = {I32: np.int32, I64: np.int64}
    for (v, nl), t in zip(cols, queries.Q1_LINEITEM_TYPES):
        assert v.shape == (n,) and v.dtype == want_dt[t] and nl is None
    flag, status = cols[0][0], cols[1][0]
    assert set(np.unique(flag)) <= {0, 1, 2}
    assert set(np.unique(status)) <= {0, 1}
    pairs = set(zip(flag.tolist(), status.tolist()))
    assert {(0, 0), (1, 1), (2, 0)} <= pairs <= {(0, 0), (1, 0), (1, 1),
                                                 (2, 0)}
    cols = queries.gen_q1_numpy(np.random.default_rng(4203), n, nulls=True)
    assert cols[0][1] is None and cols[1][1] is None
    for v, nl in cols[2:]:
        assert nl.dtype == np.uint8 and nl.shape == (n,) and 0 < nl.sum() < n


def test_abi_constants():
    assert abi.PROJ_Q1_CHARGE6 == 6
    assert C.sizeof(abi.GxAggLocalStats) == 24
    assert [f[0] for f in abi.GxAggLocalStats._fields_] == [
        "local_rows", "local_launches", "local_groups_cap", "replicas"]
    assert len(queries.Q1_SCAN_PROJS) == len(queries.Q1_SCAN_TYPES) == 7
    assert len(queries.q1_aggs()) == 8
