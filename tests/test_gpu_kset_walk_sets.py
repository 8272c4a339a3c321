"""GPU: hypo_gpu_kset_query_walk_sets (kset_kernel.hip: kset_walk_sets_kernel) against tests/kmer_vote_checker.py, as exact integers
and bytes for every site, on a set that counts, at a least count of 1, 2 and 3.

Two sets per k.  The first is case() of tests/test_gpu_kset_walks.py with every site it names: the planted differences, its `het`,
`minor` and `err` sites and the routing edges (the arrival at exactly dlo, at exactly dhi and one beyond it, dhi = 256, an N and lower
case in an anchor, an R the set does not hold).  The second, vcase(), is a truth of 3.6 kb read fifty times in error-free pieces of
100 bases, queried with the truth itself, and sites over what further reads carry another way: a base that half the reads carry
another way (two walks of about equal support); one that 2 more reads carry another way (about 40 against 2; one walk at t = 3); a
read error seen once that rejoins the path; three alleles at one base (3 walks); two two-allele bases more than k apart (exactly 4
walks: AMBIGUOUS); a three-allele and a two-allele base more than k apart (6 walks: MANY, the first 4 reported); a run of k + 1 As
(walks of several lengths, by the slack: one, four, and more than four); and a stretch that one read repeated 300 times and another
read repeated 300 times spell two ways (both supports stop at 255).  Then budgets of exactly the steps and one less, the numbers of
sites around a wave's 16 groups and a workgroup's 64, repeated and shuffled sites, the sentinel in the slots beyond n_walks and the
bytes beyond len, every refused call, and the walks entry on the same device set: the same first walk and the same NONE / UNIQUE."""
import ctypes as C
import functools

import numpy as np
import pytest

import kmer_bridge_checker as kb
import kmer_vote_checker as kv
import min_count_checker as mc
from test_gpu_kset_min_count import Counting
from test_gpu_kset_walks import D, GAP, arrays, case, other

pytestmark = pytest.mark.gpu
KS = [12, 21, 22, 31]
TS = [1, 2, 3]


@pytest.fixture(scope="module")
def gpu():
    from hypo_amd import capi
    return capi.HypoGpu(0)


@functools.lru_cache(maxsize=None)
def vcase(k):
    """(read blob, text, {name: site}, keys, counts) of one k; a site: (from, to, dlo, dhi)"""
    rng = np.random.default_rng(9100 + k)
    truth = list("".join(rng.choice(list("ACGT"), 3600)))
    hp = 2600
    truth[hp - 1:hp + k + 2] = list("C" + "A" * (k + 1) + "G")              # a run of k + 1 As
    truth = "".join(truth)
    half, extra2, once, tri, two, six, sat = 300, 500, 700, 900, 1100, 1400, 1800
    far = k + 3                                                            # no k-mer holds both bases of a pair this far apart
    alt = lambda p, n=1: truth[:p] + (other(truth[p]) if n == 1 else other(truth[p], other(truth[p]))) + truth[p + 1:]
    rc = lambda r: r.translate(str.maketrans("ACGT", "TGCA"))[::-1]
    around = lambda s, p: s[p - 50:p + 50]
    reads = []
    for j, i in enumerate(range(0, len(truth) - 99, 2)):                   # every position fifty times, both strands
        src = alt(half) if i <= half < i + 100 and j % 4 < 2 else truth    # half of the reads over `half` carry the other base
        reads.append(src[i:i + 100] if j % 2 else rc(src[i:i + 100]))
    reads += [around(alt(extra2), extra2)] * 2
    reads += [around(alt(once), once)]
    reads += [around(alt(tri), tri)] * 10 + [rc(around(alt(tri, 2), tri))] * 12
    reads += [around(alt(two), two)] * 10 + [around(alt(two + far), two + far)] * 14
    reads += [around(alt(six), six)] * 10 + [around(alt(six, 2), six)] * 12 + [around(alt(six + far), six + far)] * 14
    reads += [around(truth, sat)] * 300 + [rc(around(alt(sat), sat))] * 300
    text = truth
    sites = {}
    for name, p, q in (("half", half, half), ("extra2", extra2, extra2), ("once", once, once), ("tri", tri, tri), ("two and two", two, two + far),
                       ("three and two", six, six + far), ("saturated", sat, sat)):
        a, b = p - GAP - k, q + 1 + GAP
        sites[name] = (a, b, max(1, b - a - D), b - a + D)
    sites["only the second pair"] = (two + 2, two + far + 1 + GAP, 1, far + GAP + D)                    # L behind the first base of the pair
    a, b = hp - 3 - k, hp + k + 4                                          # the run between them: runs of k - 1 As and more are walks
    d0 = b - a
    sites.update({"run as it is": (a, b, d0, d0), "run one shorter": (a, b, d0 - 3, d0 - 2), "run four lengths": (a, b, d0 - 1, d0 + 2),
                  "run many lengths": (a, b, d0 - D, d0 + D)})
    blob = "\n".join(reads).encode()
    keys, counts = mc.read_counts(blob, k)
    return blob, text.encode(), sites, keys, counts


CASES = {"walks": case, "vote": vcase}


@functools.lru_cache(maxsize=None)
def count_map(which, k):
    blob, text, sites, keys, counts = CASES[which](k)
    return kv.count_map(keys, counts)


@functools.lru_cache(maxsize=None)
def expected(which, k, t):
    """{name: (status, steps, [(walk, low)])} at budget 4096"""
    blob, text, sites, keys, counts = CASES[which](k)
    Cm = count_map(which, k)
    return {name: kv.search_set(text[a:a + k], text[b:b + k], lo, hi, kb.BUDGET, k, Cm, t) for name, (a, b, lo, hi) in sites.items()}


def check(gpu, which, k, t, names, budget=kb.BUDGET, want=None):
    from hypo_amd import abi
    blob, text, sites, keys, counts = CASES[which](k)
    want = want or expected(which, k, t)
    status, steps, nw, ln, low, walk = gpu.kset_query_walk_sets(text, *arrays(sites, names), budget)
    assert walk.shape == (len(names), abi.KSET_MAX_WALKS, abi.KSET_MAX_WALK)
    for i, name in enumerate(names):
        st, n_steps, walks = want[name]
        assert (int(status[i]), int(steps[i]), int(nw[i])) == (st, n_steps, len(walks)), (which, k, t, name, sites[name], (status[i], steps[i], nw[i]), want[name])
        for w, (bases, c) in enumerate(walks):
            got = (int(ln[i, w]), int(low[i, w]), bytes(walk[i, w, :len(bases)]))
            assert got == (len(bases), c, bases), (which, k, t, name, w, got, (len(bases), c, bases))
            assert np.all(walk[i, w, len(bases):] == abi.WALKS_UNTOUCHED8), (which, k, t, name, w)       # bytes beyond len
        n = len(walks)                                                     # slots beyond n_walks
        assert np.all(ln[i, n:] == abi.WALKS_UNTOUCHED32) and np.all(low[i, n:] == abi.WALKS_UNTOUCHED32) and np.all(walk[i, n:] == abi.WALKS_UNTOUCHED8), (which, k, t, name)


def test_the_cases_are_what_they_are_meant_to_be():
    """on the checker alone: every named site is what its name says, and every status the entry point knows is among the cases"""
    for k in KS:
        e = {t: expected("vote", k, t) for t in TS}
        n = lambda t, name: len(e[t][name][2])
        lows = lambda t, name: [c for _, c in e[t][name][2]]
        lens = lambda t, name: [len(w) for w, _ in e[t][name][2]]
        for t in TS:
            assert e[t]["half"][0] == kb.AMBIGUOUS and n(t, "half") == 2 and min(lows(t, "half")) >= 15 and max(lows(t, "half")) - min(lows(t, "half")) <= 12
            assert e[t]["tri"][0] == kb.AMBIGUOUS and n(t, "tri") == 3 and sorted(lows(t, "tri"))[:2] == [10, 12]
            assert e[t]["two and two"][0] == kb.AMBIGUOUS and n(t, "two and two") == kv.W and sorted(lows(t, "two and two"))[:3] == [10, 10, 14]
            assert e[t]["three and two"][0] == kv.MANY and n(t, "three and two") == kv.W
            assert e[t]["only the second pair"][0] == kb.AMBIGUOUS and sorted(lows(t, "only the second pair"))[0] == 14
            assert e[t]["saturated"][0] == kb.AMBIGUOUS and lows(t, "saturated") == [255, 255]
            assert e[t]["run as it is"][0] == e[t]["run one shorter"][0] == kb.UNIQUE and lens(t, "run one shorter")[0] == lens(t, "run as it is")[0] - 2
            assert e[t]["run four lengths"][0] == kb.AMBIGUOUS and len(set(lens(t, "run four lengths"))) == kv.W
            assert e[t]["run many lengths"][0] == kv.MANY and len(set(lens(t, "run many lengths"))) == kv.W
        assert [e[t]["extra2"][0] for t in TS] == [kb.AMBIGUOUS, kb.AMBIGUOUS, kb.UNIQUE]
        assert sorted(lows(1, "extra2")) == sorted(lows(2, "extra2")) and min(lows(1, "extra2")) == 2 and max(lows(1, "extra2")) >= 30 and lows(3, "extra2")[0] >= 30
        assert [e[t]["once"][0] for t in TS] == [kb.AMBIGUOUS, kb.UNIQUE, kb.UNIQUE] and min(lows(1, "once")) == 1 and lows(2, "once")[0] >= 30
        # the walks entry's cases through this search: its three sites over what the reads carry two ways, and its routing edges
        w = {t: expected("walks", k, t) for t in TS}
        assert [w[t]["het"][0] for t in TS] == [kb.AMBIGUOUS] * 3 and len(w[1]["het"][2]) == 2
        assert [w[t]["minor"][0] for t in TS] == [kb.AMBIGUOUS, kb.AMBIGUOUS, kb.UNIQUE] and sorted(c for _, c in w[1]["minor"][2])[0] == 2
        assert w[1]["err"][0] == w[2]["err"][0] == kb.UNIQUE and w[1]["err"][1] > w[2]["err"][1]
        assert w[1]["N in L"] == w[1]["N in R"] == (kb.NOANCHOR, 0, [])
        for name, length in (("at dlo", 40), ("at dhi", 40), ("overlap one", 1), ("dhi 256", 256), ("dhi 256 wide", 200), ("lower", 15), ("lower to upper", 30)):
            assert w[1][name][0] == kb.UNIQUE and [len(x) for x, _ in w[1][name][2]] == [length], (k, name)
        for name in ("beyond dhi", "before dlo", "R not in the set", "L not in the set", "insD1", "delD1"):
            assert w[1][name][0] == kb.NONE and w[1][name][2] == [], (k, name)


@pytest.mark.parametrize("k", KS)
def test_walk_sets_equal_checker(gpu, k):
    from hypo_amd import abi
    for which in ("vote", "walks"):
        blob, text, sites, keys, counts = CASES[which](k)
        names = list(sites)
        with Counting(gpu, k, keys.size, [blob]):
            assert gpu.kset_size()[0] == keys.size
            check(gpu, which, k, 1, names)                                 # a set that counts, no threshold yet
            for t in (2, 3):
                gpu.kset_min_count(t)
                check(gpu, which, k, t, names)
            gpu.kset_min_count(1)
            rng = np.random.default_rng(k)
            check(gpu, which, k, 1, [names[i] for i in rng.permutation(len(names))] + names[:7] * 3)      # shuffled, and sites that repeat
            if which == "walks":
                continue
            for n in (1, 15, 16, 17, 63, 64, 65):                          # around a wave's 16 groups and a workgroup's 64
                check(gpu, which, k, 1, (names * 6)[:n])
            # no site: nothing is touched, whatever the pointers are
            out = gpu.kset_query_walk_sets(text, [], [], [], [], kb.BUDGET)
            assert all(a.shape[0] == 0 for a in out)
            assert gpu.lib.hypo_gpu_kset_query_walk_sets(None, C.c_uint64(0), None, None, None, None, C.c_uint32(0), C.c_uint32(0), None, None, None, None, None, None) == 0
            # a budget of exactly the steps changes nothing, one less is BUDGET with budget + 1 steps and no walk reported
            e = expected(which, k, 1)
            for name in ("half", "once", "tri", "two and two", "three and two", "run four lengths", "run many lengths", "saturated"):
                st, steps, walks = e[name]
                check(gpu, which, k, 1, [name], budget=steps)
                check(gpu, which, k, 1, [name, "tri"], budget=steps - 1, want={name: (kb.OVER_BUDGET, steps, []), "tri": kv.search_set(
                    text[sites["tri"][0]:sites["tri"][0] + k], text[sites["tri"][1]:sites["tri"][1] + k], *sites["tri"][2:], steps - 1, k, count_map(which, k), 1)})


@pytest.mark.parametrize("k", KS)
def test_first_walk_is_the_walks_entrys(gpu, k):
    """on the device alone: where neither search ends on BUDGET, the first walk and NONE / UNIQUE are hypo_gpu_kset_query_walks'"""
    from hypo_amd import abi
    for which in ("vote", "walks"):
        blob, text, sites, keys, counts = CASES[which](k)
        names = list(sites)
        with Counting(gpu, k, keys.size, [blob]):
            for t in TS:
                gpu.kset_min_count(t)
                for budget in (kb.BUDGET, 60):
                    s1, steps1, len1, walk1 = gpu.kset_query_walks(text, *arrays(sites, names), budget)
                    s2, steps2, nw, ln, low, walk = gpu.kset_query_walk_sets(text, *arrays(sites, names), budget)
                    compared = 0
                    for i, name in enumerate(names):
                        if s1[i] == abi.WALK_BUDGET or s2[i] == abi.WALK_BUDGET:
                            continue
                        compared += 1
                        assert (s1[i] == abi.WALK_NONE) == (s2[i] == abi.WALK_NONE) and (s1[i] == abi.WALK_UNIQUE) == (s2[i] == abi.WALK_UNIQUE), (which, k, t, name)
                        assert (s1[i] == abi.WALK_NOANCHOR) == (s2[i] == abi.WALK_NOANCHOR)
                        if nw[i]:
                            assert len1[i] == ln[i, 0] and bytes(walk1[i, :len1[i]]) == bytes(walk[i, 0, :ln[i, 0]]), (which, k, t, name)
                        else:
                            assert len1[i] == 0
                        if s1[i] in (abi.WALK_NONE, abi.WALK_UNIQUE):
                            assert steps1[i] == steps2[i]
                    assert budget != kb.BUDGET or compared >= len(names) // 2       # (60 visits end most of vcase()'s searches, at k = 31 all)


def test_argument_errors(gpu):
    from hypo_amd import abi
    lib = gpu.lib
    k = 12
    blob, text, sites, keys, counts = vcase(k)
    n = len(text)
    untouched = lambda out: all(np.all(a == (abi.WALKS_UNTOUCHED8 if a.dtype == np.uint8 else abi.WALKS_UNTOUCHED32)) for a in out)
    rc, *out = gpu.kset_query_walk_sets_rc(text, [0], [20], [12], [28], 100)
    assert rc == abi.HYPO_E_INVALID and b"hypo_gpu_kset_begin" in lib.hypo_gpu_last_error() and untouched(out)      # no set, as hypo_gpu_kset_query
    good = ([0, 500], [20, 530], [12, 20], [28, 40])
    # a set without counts, in the words of hypo_gpu_kset_min_count
    gpu.kset_begin(k, keys.size)
    try:
        gpu.kset_add(blob)
        assert gpu.kset_min_count_rc(2) == abi.HYPO_E_INVALID
        wording = lib.hypo_gpu_last_error()
        rc, *out = gpu.kset_query_walk_sets_rc(text, *good, 100)
        assert rc == abi.HYPO_E_INVALID and untouched(out) and lib.hypo_gpu_last_error() == wording and b"hypo_gpu_kset_counts_enable" in wording
        assert gpu.kset_query_walks_rc(text, *good, 100)[0] == 0           # (the walks entry needs none)
    finally:
        gpu.kset_end()
    with Counting(gpu, k, keys.size, [blob]):
        ok = gpu.kset_query_walk_sets(text, *good, 100)
        bad = [(([0, n - k + 1], [20, 530], [12, 20], [28, 40]), 100),     # from + k > n_bytes
               (([0, 500], [20, n - k + 1], [12, 20], [28, 40]), 100),     # to + k > n_bytes
               (([0, 2 ** 64 - 1], [20, 530], [12, 20], [28, 40]), 100),
               (([0, 500], [2 ** 64 - k, 530], [12, 20], [28, 40]), 100),
               (([0, 500], [20, 530], [12, 0], [28, 40]), 100),            # dlo < 1
               (([0, 500], [20, 530], [12, 41], [28, 40]), 100),           # dlo > dhi
               (([0, 500], [20, 530], [12, 20], [28, 257]), 100),          # dhi > HYPO_KSET_MAX_WALK
               (good, 0), (good, abi.KSET_MAX_WALK_BUDGET + 1), (good, 2 ** 32 - 1)]
        for args, budget in bad:
            rc, *out = gpu.kset_query_walk_sets_rc(text, *args, budget)
            assert rc == abi.HYPO_E_INVALID and untouched(out), (args, budget)
        rc, *out = gpu.kset_query_walk_sets_rc(text[:k - 1], [0], [0], [1], [2], 100)              # a text shorter than k
        assert rc == abi.HYPO_E_INVALID and untouched(out)
        assert gpu.kset_query_walk_sets_rc(text, [0, n - k], [n - k, 530], [1, 256], [256, 256], abi.KSET_MAX_WALK_BUDGET)[0] == 0      # the limits themselves are allowed
        # a NULL pointer
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        pos = [np.array([v], np.uint64) for v in (0, 20)]
        d = [np.array([v], np.uint32) for v in (12, 28)]
        o32 = [np.full(m, 7, np.uint32) for m in (1, 1, 1, abi.KSET_MAX_WALKS, abi.KSET_MAX_WALKS)]
        walk = np.full(abi.KSET_MAX_WALKS * abi.KSET_MAX_WALK + 1, 7, np.uint8)
        full = [text, C.c_uint64(n), p(pos[0]), p(pos[1]), p(d[0]), p(d[1]), C.c_uint32(1), C.c_uint32(100)] + [p(a) for a in o32] + [p(walk)]
        for i in (0, 2, 3, 4, 5, 8, 9, 10, 11, 12, 13):
            args = list(full)
            args[i] = None
            assert lib.hypo_gpu_kset_query_walk_sets(*args) == abi.HYPO_E_INVALID, i
            assert all(a.tolist() == [7] * a.size for a in o32 + [walk]), i
        assert lib.hypo_gpu_kset_query_walk_sets(*full) == 0
        want = kv.search_set(text[0:k], text[20:20 + k], 12, 28, 100, k, count_map("vote", k), 1)
        assert want[0] == kb.UNIQUE and len(want[2][0][0]) == 20
        assert o32[0][0] == abi.WALK_UNIQUE and o32[2][0] == 1 and o32[3].tolist() == [20, 7, 7, 7] and o32[4].tolist() == [want[2][0][1], 7, 7, 7]
        assert walk[19] != 7 and np.all(walk[20:] == 7)
        after = gpu.kset_query_walk_sets(text, *good, 100)                 # refused calls change nothing
        assert all(np.array_equal(a, b) for a, b in zip(after, ok))
