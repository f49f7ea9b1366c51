"""Sort / top-N checks that need no GPU: the CPU reference (tests/sort_ref.py)
reproduces the reference's own test vectors, the device key encoding orders
values exactly as the comparator does, and the HIP library declares and
exports the gxop_sort_* entry points."""
import ctypes
import functools
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

from galaxysql_amd.chunk import I64, I32, F64

from . import sort_ref as sr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_HEADER = os.path.join(REPO, "include", "gxop_hip.h")
HIP_SO = os.path.join(REPO, "galaxysql_amd", "csrc", "libgxhip.so")
SORT_SYMBOLS = ["gxop_sort_create", "gxop_sort_consume", "gxop_sort_build",
                "gxop_sort_next", "gxop_sort_get_stats", "gxop_sort_close"]

CASES = sr.load_golden()


def _case_rows(case):
    rows = []
    for ch in case["chunks"]:
        rows.extend(tuple(col[i] for col in ch) for i in range(len(ch[0])))
    return rows


def _limit_rows(rows, case):
    off, fetch = case["offset"], case["fetch"]
    return rows[off:] if fetch < 0 else rows[off:off + fetch]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_comparator_reproduces_golden(case):
    """The value-by-value comparator + a stable sort + offset/fetch gives
    the reference's expected rows, String cases included."""
    types = [sr._TYPE.get(t, t) for t in case["types"]]
    order = sr.golden_order(case)
    key = functools.cmp_to_key(
        lambda a, b: sr.compare_rows(a, b, order, types))
    got = _limit_rows(sorted(_case_rows(case), key=key), case)  # stable
    exp = sr.golden_expected_rows(case)
    if case["compare"] == "multiset":
        assert sorted(map(repr, got)) == sorted(map(repr, exp))
    else:
        assert got == exp


NUMERIC = [c for c in CASES if c["device"]]


@pytest.mark.parametrize("case", NUMERIC, ids=[c["name"] for c in NUMERIC])
def test_sort_ref_reproduces_golden(case):
    types, chunks = sr.golden_chunks(case)
    got = sr.columns_rows(sr.sort_ref(chunks, types, sr.golden_order(case),
                                      case["offset"], case["fetch"]))
    exp = sr.golden_expected_rows(case)
    if case["compare"] == "multiset":
        assert sorted(map(repr, got)) == sorted(map(repr, exp))
    else:
        assert got == exp


def test_string_cases_are_marked_off_device():
    off = [c["name"] for c in CASES if not c["device"]]
    assert len(off) == 3
    for c in CASES:
        has_str_key = any(c["types"][o["col"]].startswith("STR")
                          for o in c["order"])
        assert has_str_key == (not c["device"]), c["name"]


# ---- key encoding == comparator, pairwise ---------------------------------

def _nan(sign, payload):
    return sr.pack_f64((sign << 63) | (0x7ff << 52) | payload)


ADVERSARIAL = {
    I64: [-(1 << 63), (1 << 63) - 1, -1, 0, 1, -(1 << 62), 1 << 62, None],
    I32: [-(1 << 31), (1 << 31) - 1, -1, 0, 1, -(1 << 30), 1 << 30, None],
    F64: [0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308,
          float("inf"), float("-inf"), 1.0, -1.0, 1.5e300, -1.5e300,
          _nan(0, 1 << 51), _nan(1, 1 << 51), _nan(0, 12345),
          _nan(1, (1 << 51) | 77), None],
}


@pytest.mark.parametrize("btype", [I64, I32, F64])
@pytest.mark.parametrize("asc", [True, False])
def test_encode_key_orders_like_the_comparator(btype, asc):
    vals = ADVERSARIAL[btype]
    dt = {I64: np.int64, I32: np.int32, F64: np.float64}[btype]
    arr = np.array([0 if v is None else v for v in vals], dtype=dt)
    nulls = np.array([v is None for v in vals], dtype=np.uint8)
    if btype == F64:   # the NaN payloads and signs must survive numpy
        bits = sr.f64_bits(arr)
        assert len({int(b) for b, v in zip(bits, vals)
                    if v is not None and v != v}) == 4
    words, rank = sr.encode_key(arr, nulls, btype, asc)
    assert words.dtype == (np.uint32 if btype == I32 else np.uint64)
    order = [(0, asc)]
    for i, j in itertools.product(range(len(vals)), repeat=2):
        n = sr.compare_rows((vals[i],), (vals[j],), order, [btype])
        ki = (int(rank[i]), int(words[i]))
        kj = (int(rank[j]), int(words[j]))
        assert ((ki > kj) - (ki < kj)) == n, (vals[i], vals[j], asc)


def test_sort_ref_lexsort_matches_comparator_on_adversarial_values():
    """sort_perm (arithmetic sub-keys) and the comparator give the same
    stable order over every adversarial value, each listed twice."""
    for btype in (I64, I32, F64):
        vals = ADVERSARIAL[btype] * 2
        dt = {I64: np.int64, I32: np.int32, F64: np.float64}[btype]
        arr = np.array([0 if v is None else v for v in vals], dtype=dt)
        nulls = np.array([v is None for v in vals], dtype=np.uint8)
        for asc in (True, False):
            perm = sr.sort_perm([(arr, nulls)], [btype], [(0, asc)])
            key = functools.cmp_to_key(
                lambda a, b: sr.compare_rows((vals[a],), (vals[b],),
                                             [(0, asc)], [btype]))
            assert list(perm) == sorted(range(len(vals)), key=key)


# ---- the library boundary ---------------------------------------------------

@pytest.fixture(scope="module")
def hip_so():
    if not os.path.exists(HIP_SO):
        subprocess.run(["python", "-c",
                        "from galaxysql_amd.build import build_hip; "
                        "build_hip()"], check=True, cwd=REPO)
    return HIP_SO


def test_header_declares_and_hip_exports_sort_symbols(hip_so):
    txt = open(HIP_HEADER).read()
    declared = set(re.findall(r"\b(gxop_sort_[a-z_]+)\s*\(", txt))
    assert declared == set(SORT_SYMBOLS)
    lib = ctypes.CDLL(hip_so, mode=ctypes.RTLD_LOCAL)
    missing = [s for s in SORT_SYMBOLS if not hasattr(lib, s)]
    assert not missing, f"{hip_so} missing symbols: {missing}"


def test_abi_has_sort(hip_so):
    from galaxysql_amd import abi
    assert abi.load_hip().has_sort is True
    assert ctypes.sizeof(abi.GxOrderBy) == 12
    # gx_sort_cfg: two (int32 + pointer) pairs, four int64, two int32, u64
    assert ctypes.sizeof(abi.GxSortCfg) == 80
    assert ctypes.sizeof(abi.GxSortStats) == 48
