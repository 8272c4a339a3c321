"""GPU: hypo_gpu_kset_query_fixes (kset_kernel.hip: kset_fixes_kernel, kset_fixes_reduce_kernel) against tests/kmer_fix_checker.py,
as exact integers for every per-site result and every candidate's pair, for both lane-group widths the library can launch, on the
set as it is and under a least count of 2 and 3.  R and the text are those of tests/test_gpu_kset_spans.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import kmer_fix_checker as fc
import min_count_checker as mc
from test_gpu_kset_min_count import Counting
from test_gpu_kset_spans import case as span_case, group, piece  # noqa: F401  (the fixtures)

pytestmark = pytest.mark.gpu
KS = [12, 21, 22, 31]
GROUPS = [32, 64]
PER_SITE = ("none_total", "none_missing", "best_cand", "best_total", "best_missing", "zeros")


@pytest.fixture(scope="module")
def gpu():
    from hypo_amd import capi
    return capi.HypoGpu(0)


def runs_of(text, least):
    """[(first, end)] of the homopolymer runs of at least `least` bases"""
    a = np.frombuffer(text.upper(), np.uint8)
    cut = np.flatnonzero(np.concatenate([[True], a[1:] != a[:-1], [True]]))
    return [(int(b), int(e)) for b, e in zip(cut[:-1], cut[1:]) if e - b >= least and a[b] in b"ACGT"]


@functools.lru_cache(maxsize=None)
def case(k):
    """(blob, text, sets {name: (lo, hi, c0, c1)}, keys, counts, expected {(name, t): the checker's answer}), built once per k"""
    blob, R, text, _, _ = span_case(k, 2048)
    keys, counts = mc.read_counts(blob, k)
    assert np.array_equal(keys, R)
    n = len(text)
    rng = np.random.default_rng(5000 + k)
    f = k - 1                                                              # the flank a site of the host has
    site = lambda c0, c1, left=f, right=f: (max(0, c0 - left), min(n, c1 + right), c0, c1)
    edge = []
    for w in sorted({1, 2, k - 1, k, 31}):                                 # the region widths
        edge += [site(4000, 4000 + w), site(7000 + w, 7000 + 2 * w, 3, 0)]
    edge += [(0, 3 * k, 0, 1), (0, 2 * k, k - 5, k), (0, 40, 0, 31), (n - 3 * k, n, n - 1, n), (n - 2 * k, n, n - k, n - k + 3), (n - 31, n, n - 31, n)]
    edge += [(5000, 5000 + k, 5000 + k // 2, 5000 + k // 2 + 1), (5000, 5000 + k, 5000, 5000 + k), (5100, 5100 + 2 * k - 1, 5100 + k - 1, 5100 + k),
             (5200, 5200 + k - 1, 5203, 5205), (5300, 5301, 5300, 5301), (5400, 5405, 5400, 5405)]      # k bytes, 2k - 1, and too short for a window
    for length in (2047, 2048):
        edge += [(8000, 8000 + length, 8000, 8031), (8000, 8000 + length, 9000, 9001), (8000, 8000 + length, 8000 + length - 31, 8000 + length),
                 (0, length, 1290, 1310), (n - length, n, n - 40, n - 20)]
    runs = [r for r in runs_of(text, 4) if 3000 < r[0] < n - 3000][:6]
    assert len(runs) == 6
    for b, e in runs:                                                     # inside a run, at its edges, over it, just beside it
        edge += [site(b + 1, e - 1), site(b, e), site(b - 2, b + 2), site(e - 2, e + 2), site(b - 1, e + 1), site(b, b + 1), site(e - 1, e), site(e, e + 3)]
    long_runs = runs_of(text, 6)
    assert long_runs
    edge += [site(b + 1, min(e - 1, b + 32)) for b, e in long_runs[:3]]
    pal = k - k % 2
    edge += [site(998, 1003), site(1000, 1001), site(1055, 1065), site(1295, 1310), site(1320, 1330), site(1395, 1402), site(1098, 1103), site(1495, 1510),
             site(1520, 1530), site(1590, 1610), site(1695, 1710), site(1700, 1703), site(1701, 1702), site(2000, 2000 + min(pal, 31)), site(1995, 2010),
             site(2000 + pal - 3, 2000 + pal + 3)]
    edge += [site(4500, 4507)] * 3                                        # a site three times
    edge += [site(4600 + 5 * i, 4600 + 5 * i + 9) for i in range(8)]      # sites sharing bytes
    edge += [(4700, 4800, 4700 + 10 * i, 4700 + 10 * i + 10) for i in range(10)]   # one span, ten regions
    c0 = rng.integers(0, n - 31, 3000)
    w = np.where(rng.random(3000) < 0.9, rng.integers(1, 8, 3000), rng.integers(1, min(k, 31) + 1, 3000))
    left, right = rng.integers(0, k + 3, 3000), rng.integers(0, k + 3, 3000)
    rand = [site(int(a), int(a + b), int(l), int(r)) for a, b, l, r in zip(c0, w, left, right)]
    order = rng.permutation(len(rand))
    sets = {"edge": edge, "random": rand, "random shuffled": [rand[i] for i in order]}
    sets = {name: tuple(np.array([s[i] for s in v], np.uint64) for i in range(4)) for name, v in sets.items()}
    Rs = [mc.reliable_set(keys, counts, t) for t in (1, 2, 3)]
    expected = {}
    for name in ("edge", "random"):
        for t, e in zip((1, 2, 3), fc.query(text, *sets[name], k, Rs)):
            expected[(name, t)] = e
    for t in (1, 2, 3):                                                   # the shuffled sites: the same answers in another order
        e = expected[("random", t)]
        first = e["first"]
        sh = {key: [e[key][i] for i in order] for key in PER_SITE}
        for key in ("cand_total", "cand_missing"):
            sh[key] = [x for i in order for x in e[key][first[i]:first[i + 1]]]
        expected[("random shuffled", t)] = sh
    e1 = expected[("random", 1)]
    assert sum(1 for z, m in zip(e1["zeros"], e1["best_missing"]) if z == 1 and m == 0) >= 20          # the rule bites, both ways
    assert sum(1 for z in e1["zeros"] if z >= 2) >= 20 and sum(1 for z in e1["zeros"] if z == 0) >= 20
    assert expected[("random", 2)]["cand_missing"] != e1["cand_missing"] and expected[("random", 3)]["best_cand"] != e1["best_cand"]
    return blob, text, sets, keys, counts, expected


def check(gpu, text, sets, expected, t):
    for name, args in sets.items():
        exp = expected[(name, t)]
        got = gpu.kset_query_fixes(text, *args)
        for key, g in zip(PER_SITE + ("cand_total", "cand_missing"), got):
            e = np.array(exp[key], g.dtype)
            bad = np.flatnonzero(g != e) if g.shape == e.shape else None
            assert g.shape == e.shape and bad.size == 0, (t, name, key, [(int(i), int(g[i]), int(e[i])) for i in (bad[:5] if bad is not None else [])])
        nov = gpu.kset_query_fixes(text, *args, cands=False)               # cand_* NULL: the same per-site results
        assert nov[6] is None and nov[7] is None and all(np.array_equal(a, b) for a, b in zip(nov[:6], got[:6]))


@pytest.mark.parametrize("group", GROUPS, indirect=True)
@pytest.mark.parametrize("k", KS)
def test_fixes_equal_checker(gpu, k, group):
    blob, text, sets, keys, counts, expected = case(k)
    gpu.kset_begin(k, keys.size)
    try:
        gpu.kset_add(blob)
        assert gpu.kset_size()[0] == keys.size
        check(gpu, text, sets, expected, 1)
        # no site, one site, two
        lo, hi, c0, c1 = sets["edge"]
        exp = expected[("edge", 1)]
        for n in (0, 1, 2):
            got = gpu.kset_query_fixes(text, lo[:n], hi[:n], c0[:n], c1[:n])
            assert [g.tolist() for g in got[:6]] == [exp[key][:n] for key in PER_SITE]
            assert got[6].tolist() == exp["cand_total"][:exp["first"][n]] and got[7].tolist() == exp["cand_missing"][:exp["first"][n]]
    finally:
        gpu.kset_end()


@pytest.mark.parametrize("group", GROUPS, indirect=True)
@pytest.mark.parametrize("k", KS)
def test_fixes_under_a_least_count(gpu, k, group):
    blob, text, sets, keys, counts, expected = case(k)
    with Counting(gpu, k, keys.size, [blob]):
        for t in (2, 3):
            gpu.kset_min_count(t)
            check(gpu, text, sets, expected, t)
        gpu.kset_min_count(1)
        check(gpu, text, {"edge": sets["edge"]}, expected, 1)


@pytest.mark.parametrize("k", KS)
def test_candidates_equal_one_edit_variants(gpu, k):
    """every candidate of 200 sites as a site of hypo_gpu_kset_query_variants with that one edit: the same pairs"""
    blob, text, sets, keys, counts, expected = case(k)
    lo, hi, c0, c1 = (a[:200] for a in sets["random"])
    v_lo, v_hi, edit_off, eb, ee, ao, al, alts = [], [], [0], [], [], [], [], b"ACGT"
    for a, b, x, y in zip(lo.tolist(), hi.tolist(), c0.tolist(), c1.tolist()):
        for cand in fc.candidates(x, y):
            v_lo.append(a); v_hi.append(b)
            if cand[0] != "none":
                p = cand[1]
                eb.append(p); ee.append(p if cand[0] == "ins" else p + 1)
                ao.append(0 if cand[0] == "del" else b"ACGT".index(cand[2])); al.append(0 if cand[0] == "del" else 1)
            edit_off.append(len(eb))
    n_edits = np.diff(np.array(edit_off))
    var_first = np.concatenate([[0], np.cumsum(1 << n_edits)])[:-1]
    at = var_first + n_edits                                               # mask 1 of a site with an edit, mask 0 of one without
    gpu.kset_begin(k, keys.size)
    try:
        gpu.kset_add(blob)
        fixes = gpu.kset_query_fixes(text, lo, hi, c0, c1)
        var = gpu.kset_query_variants(text, alts, v_lo, v_hi, edit_off, eb, ee, ao, al)
    finally:
        gpu.kset_end()
    assert fixes[6].size == len(v_lo) >= 200 * 6
    assert np.array_equal(var[3][at], fixes[6]) and np.array_equal(var[4][at], fixes[7])
    assert 0 < int(fixes[7].sum()) < int(fixes[6].sum())


def test_argument_errors(gpu):
    from hypo_amd import abi
    lib = gpu.lib
    text = b"ACGTTGCA" * 300
    n = len(text)
    untouched = lambda out: all(np.all(a == (abi.FIXES_UNTOUCHED32 if a.dtype == np.uint32 else abi.FIXES_UNTOUCHED64)) for a in out if a is not None)
    rc, *out = gpu.kset_query_fixes_rc(text, [0], [40], [18], [22])
    assert rc == abi.HYPO_E_INVALID and b"hypo_gpu_kset_begin" in lib.hypo_gpu_last_error() and untouched(out)      # no set, as hypo_gpu_kset_query
    gpu.kset_begin(12, 100)
    try:
        gpu.kset_add(text)
        good = ([0, 100], [40, 140], [18, 110], [22, 115])
        ok = gpu.kset_query_fixes(text, *good)
        bad = [([19, 100], [40, 140], [18, 110], [22, 115]),               # lo > c0
               ([0, 100], [40, 140], [18, 110], [18, 115]),               # c0 == c1
               ([0, 100], [40, 140], [18, 116], [22, 115]),               # c0 > c1
               ([0, 100], [40, 114], [18, 110], [22, 115]),               # c1 > hi
               ([0, n - 10], [40, n + 1], [18, n - 5], [22, n - 2]),      # hi > n_bytes
               ([0, 100], [40, 140], [5, 104], [22, 136]),                # a region of 32 bytes
               ([0, 100], [40, 100 + 2049], [18, 110], [22, 115]),        # a span of 2049 bytes
               ([2 ** 63], [2 ** 63 + 40], [2 ** 63 + 10], [2 ** 63 + 12]),
               ([0], [2 ** 64 - 1], [10], [12])]
        for args in bad:
            rc, *out = gpu.kset_query_fixes_rc(text, *args)
            assert rc == abi.HYPO_E_INVALID and untouched(out), args
        assert gpu.kset_query_fixes_rc(text, [0, 100], [40, 100 + 2048], [5, 104], [36, 135])[0] == 0      # 31 and 2048 are allowed
        # a required NULL pointer, and one of cand_* without the other
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        pos = [np.array([v], np.uint64) for v in (0, 40, 18, 22)]
        o64 = [np.full(1, 7, np.uint64) for _ in range(4)]
        o32 = [np.full(1, 7, np.uint32) for _ in range(2)]
        cand = [np.full(34, 7, np.uint64) for _ in range(2)]                 # 9 * 4 - 3 candidates and one more
        full = [text, C.c_uint64(n), p(pos[0]), p(pos[1]), p(pos[2]), p(pos[3]), C.c_uint32(1), p(o64[0]), p(o64[1]), p(o32[0]), p(o64[2]), p(o64[3]), p(o32[1]),
                p(cand[0]), p(cand[1])]
        for i in (0, 2, 3, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14):
            args = list(full)
            args[i] = None
            assert lib.hypo_gpu_kset_query_fixes(*args) == abi.HYPO_E_INVALID, i
            assert all(a.tolist() == [7] * a.size for a in o64 + o32 + cand), i
        none = list(full)
        none[6] = C.c_uint32(0)
        for i in (0, 2, 3, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14):
            none[i] = None
        assert lib.hypo_gpu_kset_query_fixes(*none) == 0                   # no site: nothing to do, nothing touched
        assert lib.hypo_gpu_kset_query_fixes(*full) == 0 and cand[0][0] != 7 and cand[0][32] != 7 and cand[0][33] == 7 and o32[0][0] != 7
        after = gpu.kset_query_fixes(text, *good)                          # refused calls change nothing
        assert all(np.array_equal(a, b) for a, b in zip(after, ok))
    finally:
        gpu.kset_end()
