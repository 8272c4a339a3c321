"""GPU: hypo_gpu_kset_query_walks (kset_kernel.hip: kset_walks_kernel, kset_walks_min_kernel) against tests/kmer_bridge_checker.py, as
exact integers and bytes for every site, on the set as it is and under a least count of 2 and 3.

The reads are error-free pieces of a truth string of a few kb, every position fifty times.  The queried text is the truth with planted
differences, each with a site around it whose anchors lie 2 bases off the difference: one substitution; insertions and deletions of
1, 2 and D = 8 bases; a length change of D + 1 either way (NONE); two substitutions 3 apart; a homopolymer run and a dinucleotide
repeat one unit short.  Three places where the text is the truth: a base that half the reads carry another way (AMBIGUOUS at every t
tried), one that two more reads carry another way (AMBIGUOUS, and UNIQUE at t = 3, above that allele's count), and a read error seen
once that ends a few bases on (more steps at t = 1, none of them at t = 2).  Then the routing edges: the arrival at exactly dlo, at
exactly dhi and one beyond it, anchors that overlap, dhi = 256, a budget of exactly the steps and one less, an N and lower case in an
anchor, an R the set does not hold, from == to, repeated and shuffled sites, the numbers of sites around a wave's 16 groups, no site,
and every refused call."""
import ctypes as C
import functools

import numpy as np
import pytest

import kmer_bridge_checker as kb
import min_count_checker as mc
from test_gpu_kset_min_count import Counting

pytestmark = pytest.mark.gpu
KS = [12, 21, 22, 31]
TS = [1, 2, 3]
D = 8
GAP = 2                                                                    # bases between a planted difference and either anchor


@pytest.fixture(scope="module")
def gpu():
    from hypo_amd import capi
    return capi.HypoGpu(0)


def other(c, *more):
    return next(x for x in "ACGT" if x != c and x not in more)


@functools.lru_cache(maxsize=None)
def case(k):
    """(read blob, text, {name: site}, keys, counts) of one k; a site: (from, to, dlo, dhi)"""
    rng = np.random.default_rng(9000 + k)
    rnd = lambda n: "".join(rng.choice(list("ACGT"), n))
    truth = list(rnd(4200))
    truth[1600:1610] = list("C" + "A" * 8 + "G")                           # a homopolymer run
    truth[1750:1762] = list("T" + "AC" * 5 + "G")                          # a dinucleotide repeat
    truth = "".join(truth)
    het, minor, err = 3000, 3150, 3300
    alt = lambda p: truth[:p] + other(truth[p]) + truth[p + 1:]
    rc = lambda r: r.translate(str.maketrans("ACGT", "TGCA"))[::-1]
    reads = []
    for j, i in enumerate(range(0, len(truth) - 99, 2)):                   # every position fifty times, both strands
        src = alt(het) if i <= het < i + 100 and j % 4 < 2 else truth      # half of the reads over `het` carry the other base
        reads.append(src[i:i + 100] if j % 2 else rc(src[i:i + 100]))
    reads += [alt(minor)[minor - 50:minor + 50]] * 2                       # two more reads carry `minor` another way
    reads.append(alt(err)[err - 60:err + 4])                               # a read error seen once, 3 bases before its read ends
    # the text: the truth with planted differences, from the last to the first so that the positions stay the truth's
    plants = {}                                                            # name: (position, bases of the truth that go, bases that come)
    at = 200
    for name, gone, come in [("sub", 1, None), ("ins1", 0, 1), ("ins2", 0, 2), ("insD", 0, D), ("insD1", 0, D + 1), ("del1", 1, 0), ("del2", 2, 0), ("delD", D, 0),
                             ("delD1", D + 1, 0), ("subs3", 4, None)]:
        if come is None:                                                   # substitutions at the first and the last of the bases that go
            new = other(truth[at]) + truth[at + 1:at + gone - 1] + (other(truth[at + gone - 1]) if gone > 1 else "")
        else:
            new = rnd(come)
        plants[name] = (at, gone, new)
        at += 130
    plants["hp"] = (1601, 1, "")
    plants["dinuc"] = (1751, 2, "")
    text = truth
    sites = {}
    for name, (p, gone, new) in sorted(plants.items(), key=lambda x: -x[1][0]):
        text = text[:p] + new + text[p + gone:]
    shift = 0
    for name, (p, gone, new) in sorted(plants.items(), key=lambda x: x[1][0]):
        lo, hi = p, p + gone                                               # the truth's bases that differ
        if name in ("hp", "dinuc"):                                        # the whole run is where the difference can lie
            lo, hi = (1601, 1609) if name == "hp" else (1751, 1761)
        a = lo + shift - GAP - k
        b = hi + shift + (len(new) - gone) + GAP
        d0 = b - a
        sites[name] = (a, b, max(1, d0 - D), d0 + D)
        shift += len(new) - gone
    assert shift == 0 + 1 + 2 + D + D + 1 - 1 - 2 - D - D - 1 - 1 - 2
    tail = shift                                                           # what lies behind the plants is the truth, `tail` further on
    for name, p in (("het", het), ("minor", minor), ("err", err)):
        a, b = p + tail - GAP - k, p + tail + 1 + GAP
        sites[name] = (a, b, max(1, b - a - D), b - a + D)
    # routing edges, on a stretch where the text is the truth
    e = 3500 + tail
    sites.update({"at dlo": (e, e + 40, 40, 45), "at dhi": (e, e + 40, 35, 40), "beyond dhi": (e, e + 40, 34, 39), "before dlo": (e, e + 40, 41, 48),
                  "overlap": (e, e + 3, 1, 9), "overlap one": (e + 1, e + 2, 1, 1), "dhi 256": (e, e + 256, 250, 256), "dhi 256 wide": (e, e + 200, 1, 256),
                  "beyond 256": (e - 10, e + 250, 200, 256), "same": (e, e, 1, 30), "backwards": (e + 30, e, 1, 60)})
    t = list(text)
    t[e + 300 + k // 2] = "N"                                              # an N inside an anchor
    t[e + 340:e + 400] = list("".join(t[e + 340:e + 400]).lower())         # lower-case anchors and what lies between them
    sites.update({"N in L": (e + 300, e + 330, 20, 40), "N in R": (e + 270, e + 300 + k // 2 - k + 1, 1, 60), "lower": (e + 345, e + 360, 10, 20),
                  "lower to upper": (e + 380, e + 410, 25, 35)})
    text = "".join(t) + rnd(300)                                           # and a stretch the reads have never seen
    n = len(text)
    sites.update({"R not in the set": (e, n - 200, 1, 256), "L not in the set": (n - 200, e, 1, 256), "first bytes": (0, 20, 12, 28), "last bytes": (n - k - 5, n - k, 1, 10)})
    blob = "\n".join(reads).encode()
    keys, counts = mc.read_counts(blob, k)
    return blob, text.encode(), sites, keys, counts


@functools.lru_cache(maxsize=None)
def expected(k, t):
    """{name: (status, steps, walk)} at budget 4096"""
    blob, text, sites, keys, counts = case(k)
    R = kb.as_set(mc.reliable_set(keys, counts, t))
    return {name: kb.search(text[a:a + k], text[b:b + k], lo, hi, kb.BUDGET, k, R) for name, (a, b, lo, hi) in sites.items()}


def arrays(sites, names):
    cols = list(zip(*[sites[n] for n in names]))
    return np.array(cols[0], np.uint64), np.array(cols[1], np.uint64), np.array(cols[2], np.uint32), np.array(cols[3], np.uint32)


def check(gpu, k, t, names, budget=kb.BUDGET, want=None):
    from hypo_amd import abi
    blob, text, sites, keys, counts = case(k)
    want = want or expected(k, t)
    status, steps, ln, walk = gpu.kset_query_walks(text, *arrays(sites, names), budget)
    for i, name in enumerate(names):
        st, n_steps, w = want[name]
        got = (int(status[i]), int(steps[i]), int(ln[i]), bytes(walk[i, :len(w)]))
        assert got == (st, n_steps, len(w), w), (k, t, name, sites[name], got, (st, n_steps, len(w), w))
        assert np.all(walk[i, len(w):] == abi.WALKS_UNTOUCHED8), (k, t, name)       # (this library leaves what lies beyond len alone)


def test_the_cases_are_what_they_are_meant_to_be():
    """on the checker alone: the planted differences come back as the truth, and every status the entry point knows is among the cases"""
    for k in KS:
        blob, text, sites, keys, counts = case(k)
        e = {t: expected(k, t) for t in TS}
        for name in ("sub", "ins1", "ins2", "insD", "del1", "del2", "delD", "subs3", "hp", "dinuc"):
            for t in TS:
                assert e[t][name][0] == kb.UNIQUE, (k, t, name, e[t][name])
        for name in ("insD1", "delD1", "beyond dhi", "before dlo", "R not in the set", "L not in the set", "beyond 256"):
            assert e[1][name][0] == kb.NONE and e[1][name][2] == b"", (k, name, e[1][name])
        assert [e[t]["het"][0] for t in TS] == [kb.AMBIGUOUS] * 3
        assert [e[t]["minor"][0] for t in TS] == [kb.AMBIGUOUS, kb.AMBIGUOUS, kb.UNIQUE]
        assert e[1]["err"][0] == e[2]["err"][0] == kb.UNIQUE and e[1]["err"][2] == e[2]["err"][2] and e[1]["err"][1] > e[2]["err"][1]
        assert e[1]["N in L"] == e[1]["N in R"] == (kb.NOANCHOR, 0, b"")
        for name, n in (("at dlo", 40), ("at dhi", 40), ("overlap", 3), ("overlap one", 1), ("dhi 256", 256), ("dhi 256 wide", 200), ("lower", 15), ("lower to upper", 30)):
            assert e[1][name][0] == kb.UNIQUE and len(e[1][name][2]) == n, (k, name, e[1][name])
        a, b, lo, hi = sites["sub"]
        assert (text[:a + k] + e[1]["sub"][2]).upper() != text[:b + k].upper()
        assert e[1]["L not in the set"][1] == 1 and e[1]["R not in the set"][1] > 256


@pytest.mark.parametrize("k", KS)
def test_walks_equal_checker(gpu, k):
    blob, text, sites, keys, counts = case(k)
    names = list(sites)
    gpu.kset_begin(k, keys.size)
    try:
        gpu.kset_add(blob)
        assert gpu.kset_size()[0] == keys.size
        check(gpu, k, 1, names)
        rng = np.random.default_rng(k)
        check(gpu, k, 1, [names[i] for i in rng.permutation(len(names))] + names[:7] * 3)      # shuffled, and sites that repeat
        for n in (1, 15, 16, 17, 64, 65):                                   # around a wave's 16 groups and a workgroup's 64
            check(gpu, k, 1, (names * 3)[:n])
        # no site: nothing is touched, whatever the pointers are
        out = gpu.kset_query_walks(text, [], [], [], [], kb.BUDGET)
        assert all(a.size == 0 for a in out)
        assert gpu.lib.hypo_gpu_kset_query_walks(None, C.c_uint64(0), None, None, None, None, C.c_uint32(0), C.c_uint32(0), None, None, None, None) == 0
        # a budget of exactly the steps changes nothing, one less is BUDGET with budget + 1 steps and no walk
        e = expected(k, 1)
        for name in ("sub", "delD", "het", "err", "dhi 256", "insD1", "overlap one"):
            st, steps, w = e[name]
            check(gpu, k, 1, [name], budget=steps)
            if steps > 1:
                check(gpu, k, 1, [name], budget=steps - 1, want={name: (kb.OVER_BUDGET, steps, b"")})
        check(gpu, k, 1, ["L not in the set"], budget=1)
        st, steps, w = e["R not in the set"]
        check(gpu, k, 1, ["R not in the set", "sub"], budget=100, want={"R not in the set": (kb.OVER_BUDGET, 101, b""), "sub": e["sub"]})
    finally:
        gpu.kset_end()


@pytest.mark.parametrize("k", KS)
def test_walks_under_a_least_count(gpu, k):
    blob, text, sites, keys, counts = case(k)
    names = list(sites)
    with Counting(gpu, k, keys.size, [blob]):
        check(gpu, k, 1, names)                                            # a set that counts, no threshold yet
        for t in (2, 3):
            gpu.kset_min_count(t)
            check(gpu, k, t, names)
        gpu.kset_min_count(1)
        check(gpu, k, 1, names[:20])


def test_argument_errors(gpu):
    from hypo_amd import abi
    lib = gpu.lib
    k = 12
    blob, text, sites, keys, counts = case(k)
    n = len(text)
    untouched = lambda out: all(np.all(a == (abi.WALKS_UNTOUCHED8 if a.dtype == np.uint8 else abi.WALKS_UNTOUCHED32)) for a in out)
    rc, *out = gpu.kset_query_walks_rc(text, [0], [20], [12], [28], 100)
    assert rc == abi.HYPO_E_INVALID and b"hypo_gpu_kset_begin" in lib.hypo_gpu_last_error() and untouched(out)      # no set, as hypo_gpu_kset_query
    gpu.kset_begin(k, keys.size)
    try:
        gpu.kset_add(blob)
        good = ([0, 500], [20, 530], [12, 20], [28, 40])
        ok = gpu.kset_query_walks(text, *good, 100)
        bad = [(([0, n - k + 1], [20, 530], [12, 20], [28, 40]), 100),     # from + k > n_bytes
               (([0, 500], [20, n - k + 1], [12, 20], [28, 40]), 100),     # to + k > n_bytes
               (([0, 2 ** 64 - 1], [20, 530], [12, 20], [28, 40]), 100),
               (([0, 500], [2 ** 64 - k, 530], [12, 20], [28, 40]), 100),
               (([0, 500], [20, 530], [12, 0], [28, 40]), 100),            # dlo < 1
               (([0, 500], [20, 530], [12, 41], [28, 40]), 100),           # dlo > dhi
               (([0, 500], [20, 530], [12, 20], [28, 257]), 100),          # dhi > HYPO_KSET_MAX_WALK
               (good, 0), (good, abi.KSET_MAX_WALK_BUDGET + 1), (good, 2 ** 32 - 1)]
        for args, budget in bad:
            rc, *out = gpu.kset_query_walks_rc(text, *args, budget)
            assert rc == abi.HYPO_E_INVALID and untouched(out), (args, budget)
        rc, *out = gpu.kset_query_walks_rc(text[:k - 1], [0], [0], [1], [2], 100)                  # a text shorter than k
        assert rc == abi.HYPO_E_INVALID and untouched(out)
        assert gpu.kset_query_walks_rc(text, [0, n - k], [n - k, 530], [1, 256], [256, 256], abi.KSET_MAX_WALK_BUDGET)[0] == 0      # the limits themselves are allowed
        # a NULL pointer
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        pos = [np.array([v], np.uint64) for v in (0, 20)]
        d = [np.array([v], np.uint32) for v in (12, 28)]
        o32 = [np.full(1, 7, np.uint32) for _ in range(3)]
        walk = np.full(abi.KSET_MAX_WALK + 1, 7, np.uint8)
        full = [text, C.c_uint64(n), p(pos[0]), p(pos[1]), p(d[0]), p(d[1]), C.c_uint32(1), C.c_uint32(100), p(o32[0]), p(o32[1]), p(o32[2]), p(walk)]
        for i in (0, 2, 3, 4, 5, 8, 9, 10, 11):
            args = list(full)
            args[i] = None
            assert lib.hypo_gpu_kset_query_walks(*args) == abi.HYPO_E_INVALID, i
            assert all(a.tolist() == [7] * a.size for a in o32 + [walk]), i
        assert lib.hypo_gpu_kset_query_walks(*full) == 0 and o32[0][0] == abi.WALK_UNIQUE and o32[2][0] == 20 and walk[19] != 7 and walk[abi.KSET_MAX_WALK] == 7
        after = gpu.kset_query_walks(text, *good, 100)                     # refused calls change nothing
        assert all(np.array_equal(a, b) for a, b in zip(after, ok))
    finally:
        gpu.kset_end()
