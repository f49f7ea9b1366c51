"""Reference for the exact DECIMAL SUM / AVG aggregates (GX_AGG_SUM_DEC /
GX_AGG_AVG_DEC): Python big-integer arithmetic, no tolerance anywhere.

Values travel as Python ints scaled by 10^scale (None = NULL). A result is a
multiset of rows; a DECIMAL cell is compared as (scaled value, scale), a NULL
cell as None. Records are decoded twice: by chunk.dec40_decode_wide and by
decode_general below, written independently from the DecimalStructure layout
(DecimalTypeBase.java:61-65,101-102), and the two must agree."""
import json
import os
from collections import Counter

import numpy as np

from galaxysql_amd.chunk import (Block, Chunk, DECIMAL, dec40_decode_wide,
                                 dec40_encode_wide)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "decsum_vectors.json")
WORD = 1_000_000_000


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


def decode_general(p):
    """(scaled, scale) of one 40-B record, digit-position arithmetic: integer
    word k of iw weighs 10^(9(iw-1-k)); fraction word j weighs 10^-(9(j+1)),
    the last one carrying its digits left-aligned (trailing zeros up to 9)."""
    p = bytes(p)
    integers, fractions, neg = p[36], p[37], p[39]
    iw = -(-integers // 9)
    fw = -(-fractions // 9)
    assert iw + fw <= 9, "record holds 9 words"
    words = [int.from_bytes(p[4 * k:4 * k + 4], "little", signed=True)
             for k in range(iw + fw)]
    assert all(0 <= w < WORD for w in words)
    scaled = 0
    for k in range(iw):
        scaled += words[k] * 10 ** (9 * (iw - 1 - k) + fractions)
    for j in range(fw):
        shift = fractions - 9 * (j + 1)   # >= 0 except for the last word
        w = words[iw + j]
        if shift >= 0:
            scaled += w * 10 ** shift
        else:
            assert w % 10 ** (-shift) == 0, "fraction word not left-aligned"
            scaled += w // 10 ** (-shift)
    return (-scaled if neg else scaled), fractions


def decode_cell(p):
    a = dec40_decode_wide(p)
    b = decode_general(p)
    assert a == b, (a, b, bytes(p).hex())
    return a


def ref_sum(keys, vals, scale):
    """{key: (sum, scale) or None}; keys None = global aggregate (key ())."""
    out = {}
    for i, v in enumerate(vals):
        k = () if keys is None else keys[i]
        cur = out.setdefault(k, None)
        if v is not None:
            out[k] = (0 if cur is None else cur) + int(v)
    if keys is None and not out:
        out[()] = None
    return {k: None if s is None else (s, scale) for k, s in out.items()}


def avg4(total, count, scale):
    """round_half_up(total x 10^-scale / count, 4) as a scale-4 integer,
    rounding the magnitude; integer arithmetic only."""
    num = abs(total) * 10 ** (4 - scale)
    q = (2 * num + count) // (2 * count)
    return -q if total < 0 else q


def ref_avg(keys, vals, scale):
    sums, counts = {}, {}
    for i, v in enumerate(vals):
        k = () if keys is None else keys[i]
        sums.setdefault(k, 0)
        counts.setdefault(k, 0)
        if v is not None:
            sums[k] += int(v)
            counts[k] += 1
    if keys is None and not sums:
        sums[()] = counts[()] = 0
    return {k: None if counts[k] == 0 else (avg4(sums[k], counts[k], scale), 4)
            for k in sums}


def result_rows(chunks):
    """Rows of result chunks with DECIMAL cells decoded to (scaled, scale)."""
    rows = []
    for c in chunks:
        for r in c.rows():
            rows.append(tuple(
                decode_cell(v) if b.type == DECIMAL and v is not None else v
                for v, b in zip(r, c.blocks)))
    return rows


def expected_rows(*per_agg):
    """Join {key: cell} dicts (one per aggregate, same key set) into rows
    key + cells; key is a tuple (empty for the global aggregate)."""
    keys = per_agg[0].keys()
    for d in per_agg[1:]:
        assert d.keys() == keys
    return [tuple(k) + tuple(d[k] for d in per_agg) for k in keys]


def same(got_rows, want_rows):
    assert len(got_rows) == len(want_rows), (len(got_rows), len(want_rows))
    got, want = Counter(got_rows), Counter(want_rows)
    if got != want:
        diff = list((want - got).items())[:5], list((got - want).items())[:5]
        raise AssertionError(f"rows differ (missing, unexpected): {diff}")


def dec_block(vals, scale_of=None, scale=0):
    """DECIMAL Block of scaled ints (None = NULL) encoded at `scale`, or at a
    per-value scale scale_of[i] (the value is then given at THAT scale)."""
    n = len(vals)
    recs = np.zeros((n, 40), dtype=np.uint8)
    nulls = np.zeros(n, dtype=np.uint8)
    for i, v in enumerate(vals):
        if v is None:
            nulls[i] = 1
            continue
        s = scale if scale_of is None else scale_of[i]
        recs[i] = np.frombuffer(dec40_encode_wide(int(v), s), dtype=np.uint8)
    return Block(DECIMAL, values=recs, nulls=nulls if nulls.any() else None)


def split_chunks(blocks_fn, n, chunk_size):
    """Chunks over [0, n) in steps of chunk_size; blocks_fn(a, b) -> blocks."""
    return [Chunk(blocks_fn(a, min(a + chunk_size, n)))
            for a in range(0, n, chunk_size)]
