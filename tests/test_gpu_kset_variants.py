"""GPU: hypo_gpu_kset_query_variants (kset_kernel.hip, the variants kernel and its reduction) against qv_checker.seq_stats of every
variant's Python-built string and guard_records_checker.best, as exact integers, for both lane-group widths.  R and the text are
those of tests/test_gpu_kset_spans.py (26 kb)."""
import ctypes as C
import os

import numpy as np
import pytest

import guard_records_checker as grc
import qv_checker as qc
from test_gpu_kset_spans import case

pytestmark = pytest.mark.gpu
KS = [12, 21, 22, 31]
GROUPS = [32, 64]


@pytest.fixture(scope="module")
def gpu():
    from hypo_amd import capi
    return capi.HypoGpu(0)


@pytest.fixture
def group(request):
    old = os.environ.get("HYPO_KSET_SPAN_GROUP")
    os.environ["HYPO_KSET_SPAN_GROUP"] = str(request.param)
    yield request.param
    if old is None:
        del os.environ["HYPO_KSET_SPAN_GROUP"]
    else:
        os.environ["HYPO_KSET_SPAN_GROUP"] = old


class Sites:
    """sites [(lo, hi, [(eb, ee, alt bytes)])] as the arrays of the entry point; every ALT gets bytes of its own in `alts`"""

    def __init__(self, sites):
        self.sites = sites
        alts, eb, ee, ao, al, eoff = bytearray(b"#"), [], [], [], [], [0]      # (a byte no ALT owns in front)
        for lo, hi, edits in sites:
            for b, e, alt in edits:
                eb.append(b); ee.append(e); ao.append(len(alts)); al.append(len(alt))
                alts += alt + b"#"
            eoff.append(len(eb))
        self.alts = bytes(alts)
        self.lo, self.hi = np.array([s[0] for s in sites], np.uint64), np.array([s[1] for s in sites], np.uint64)
        self.eoff, self.al = np.array(eoff, np.uint32), np.array(al, np.uint32)
        self.eb, self.ee, self.ao = (np.array(x, np.uint64) for x in (eb, ee, ao))

    def args(self):
        return self.alts, self.lo, self.hi, self.eoff, self.eb, self.ee, self.ao, self.al

    def strings(self, text):
        return [grc.site_variants(text, self.alts, lo, hi, [(b, e, o, len(a)) for (b, e, a), o in zip(edits, self.ao[i0:].tolist())])
                for (lo, hi, edits), i0 in zip(self.sites, self.eoff.tolist())]


def random_site(rng, lo, hi, n, letters=b"ACGT"):
    """n ascending, non-overlapping edits inside [lo, hi): REF and ALT of 0..3 bytes each"""
    cuts = np.sort(rng.integers(lo, hi + 1, 2 * n)).tolist()
    edits = []
    for j in range(n):
        b = cuts[2 * j]
        e = min(cuts[2 * j + 1], b + int(rng.integers(0, 4)))
        edits.append((b, e, bytes(rng.choice(list(letters), int(rng.integers(0, 4))).tolist())))
    return (lo, hi, edits)


_sets = {}


def site_sets(k, piece):
    """{name: (Sites, per site [(total, missing) per mask])} of one k, built once and shared by both group widths"""
    if k in _sets:
        return _sets[k]
    blob, R, text, _, _ = case(k, piece)
    n = len(text)
    rng = np.random.default_rng(9000 + k)
    W = lambda w: w + k - 1                                            # the length of a text with w windows
    edge = []
    for ne in (0, 1, 2, 3, 8):                                         # numbers of edits (12 is a set of its own below)
        edge += [random_site(rng, a, a + 90 + ne, ne) for a in (300 + 7 * ne, 7000 + ne)]
    a = 3000
    edge += [(a, a + 80, [(a + 10, a + 10, b"ACG"), (a + 20, a + 25, b""), (a + 30, a + 30, b""), (a + 40, a + 41, b"T")]),   # empty REF, empty ALT, both empty
             (a, a + 80, [(a + 10, a + 12, b"A"), (a + 12, a + 12, b"GG"), (a + 12, a + 15, b""), (a + 15, a + 16, b"C")]),   # abutting edits
             (a, a + 80, [(a, a + 2, b"TTT"), (a + 78, a + 80, b"G")]),                                                      # one at lo, one ending at hi
             (a, a + 80, [(a, a, b"C"), (a + 80, a + 80, b"AC")]),                                                           # insertions at lo and at hi
             (a, a + 80, [(a + 20, a + 21, b"N"), (a + 30, a + 32, b"acgt"), (a + 50, a + 50, b"RYK"), (a + 60, a + 61, b"g")]),
             (1290, 1410, [(1295, 1300, b"ACGTAC"), (1400, 1405, b"N")]),                                                    # edits inside and beside the N run
             (a, a + k + 2, [(a + 3, a + 8, b""), (a + 9, a + 10, b"")]),                                                    # ALTs that make it shorter than k
             (a, a + k - 1, [(a + 1, a + 1, b"A"), (a + 2, a + 2, b"CG")]),                                                  # no window without an edit
             (n - 50, n, [(n - 1, n, b"A"), (n, n, b"CC")]), (0, 40, [(0, 1, b""), (1, 1, b"T")]), (n, n, []), (0, 0, [(0, 0, b"ACGT" * 8)])]
    # window counts around the pass boundaries of both widths for some masks and not for others: an insertion of 3, a deletion of 2
    for w in (0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129):
        a = 8000 + 13 * w
        L = W(w) if w else k - 1
        edge.append((a, a + L, [(a + L // 2, a + L // 2, b"GAT")]))
        edge.append((a, a + L + 2, [(a + L // 2, a + L // 2 + 2, b""), (a + 1, a + 2, b"A")][::-1]))
    # an edit boundary exactly on a pass boundary (byte 32, 64, 128 of the variant), with an ALT as long as a pass
    for g in (32, 64):
        a = 12000 + g
        edge.append((a, a + 4 * g, [(a + g, a + g + 1, bytes(text[500:500 + g])), (a + 2 * g, a + 2 * g, b"A"), (a + 3 * g - 1, a + 3 * g, b"")]))
        edge.append((a, a + 4 * g, [(a + g - 5, a + g, b""), (a + g, a + g, b"ACGTA")]))
    edge += [random_site(np.random.default_rng(1), 4000, 4090, 2)] * 3                                   # identical
    edge += [(5000, 5200, [(5100, 5101, b"C")]), (5010, 5190, [(5100, 5101, b"C")]), (5090, 5090 + k, [(5100, 5101, b"C")])]   # nested
    order = rng.permutation(len(edge))
    twelve = [random_site(rng, 15000, 15100, 12), (16000, 16060, [(16000 + 5 * j, 16000 + 5 * j + 1, b"ACGT"[j % 4:j % 4 + 1]) for j in range(12)])]
    short = [random_site(rng, int(a), int(a) + int(rng.integers(40, 61)), int(rng.integers(1, 3))) for a in rng.integers(0, n - 60, 2000)]
    long_site = (100, 20100, [(150, 151, b"T"), (10000, 10004, b""), (20050, 20050, b"ACGTACGTAC")])
    plain = [(int(a), int(a) + 50 + i % 7, []) for i, a in enumerate(rng.integers(0, n - 60, 9))]       # one variant each
    sets = {"edge": edge, "edge shuffled": [edge[i] for i in order], "twelve": twelve,
            "one long among short": short[:1000] + [long_site] + short[1000:], "plain": plain}
    memo = {}

    def ref(s):
        if s not in memo:
            memo[s] = qc.seq_stats(s, k, R)
        return memo[s]
    out = {}
    for name, sites in sets.items():
        S = Sites(sites)
        out[name] = (S, [[ref(v) for v in vs] for vs in S.strings(text)])
    counts = {m for w in out["edge"][1] for _, m in w} | {t for w in out["edge"][1] for t, _ in w}
    assert {0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129} <= counts
    assert any(len({t for t, _ in w}) > 1 for w in out["edge"][1])
    _sets[k] = out
    return out


def expect(want):
    """(best_mask, best_total, best_missing, var_total, var_missing) from per-site [(total, missing) per mask]"""
    best = [grc.best([m for _, m in w]) for w in want]
    return (np.array(best, np.uint32), np.array([w[b][0] for w, b in zip(want, best)], np.uint64), np.array([w[b][1] for w, b in zip(want, best)], np.uint64),
            np.array([t for w in want for t, _ in w], np.uint64), np.array([m for w in want for _, m in w], np.uint64))


@pytest.mark.parametrize("group", GROUPS, indirect=True)
@pytest.mark.parametrize("k", KS)
def test_variants_equal_checker(gpu, k, group):
    from hypo_amd import capi
    blob, R, text, _, _ = case(k, capi.KSET_SPAN_PIECE)
    sets = site_sets(k, capi.KSET_SPAN_PIECE)
    gpu.kset_begin(k, R.size)
    try:
        gpu.kset_add(blob)
        assert gpu.kset_size()[0] == R.size
        for name, (S, want) in sets.items():
            exp = expect(want)
            got = gpu.kset_query_variants(text, *S.args())
            for what, g, e in zip(("best_mask", "best_total", "best_missing", "var_total", "var_missing"), got, exp):
                bad = np.flatnonzero(g != e)
                assert g.shape == e.shape and bad.size == 0, (name, what, [(int(i), int(g[i]), int(e[i])) for i in bad[:5]])
            again = gpu.kset_query_variants(text, *S.args())                             # the same input gives the same arrays
            assert all(np.array_equal(a, b) for a, b in zip(again, got))
            nov = gpu.kset_query_variants(text, *S.args(), variants=False)               # var_* NULL: the same best_*
            assert nov[3] is None and nov[4] is None and all(np.array_equal(a, b) for a, b in zip(nov[:3], got[:3]))
        assert len(sets["twelve"][1][0]) == 4096 and max(len(w) for w in sets["edge"][1]) == 256
        S, want = sets["one long among short"]
        assert want[1000][0][0] > 9 * capi.KSET_SPAN_PIECE                               # pieces were cut
        # variant 0 is the span [lo, hi), the last variant the string with every edit applied
        S, want = sets["edge"]
        vt, vm = gpu.kset_query_variants(text, *S.args())[3:]
        first = np.concatenate([[0], np.cumsum([len(w) for w in want])])
        ts, ms = gpu.kset_query_spans(text, S.lo, S.hi)
        assert ts.tolist() == vt[first[:-1]].tolist() and ms.tolist() == vm[first[:-1]].tolist()
        tq, mq = gpu.kset_query([v[-1] for v in S.strings(text)])
        assert tq.tolist() == vt[first[1:] - 1].tolist() and mq.tolist() == vm[first[1:] - 1].tolist()
        # n_sites of 0, 1 and one more than a workgroup's share (256 lanes / the group width items, one item a site)
        S, want = sets["plain"]
        for n in (0, 1, 256 // group, 256 // group + 1):
            sub = Sites(S.sites[:n])
            got = gpu.kset_query_variants(text, *sub.args())
            assert all(g.tolist() == e.tolist() for g, e in zip(got, expect(want[:n])))
        # a text shorter than k, and an empty one
        tiny = Sites([(0, 4, [(1, 2, b"")]), (1, 3, [])])
        assert [x.tolist() for x in gpu.kset_query_variants(b"ACGT", *tiny.args())] == [[1, 0], [0, 0], [0, 0], [0, 0, 0], [0, 0, 0]]
        assert [x.tolist() for x in gpu.kset_query_variants(b"", *Sites([(0, 0, [])]).args())] == [[0], [0], [0], [0], [0]]
    finally:
        gpu.kset_end()


def test_argument_errors(gpu):
    from hypo_amd import abi, capi
    lib = gpu.lib
    text = b"ACGTTGCA" * 8
    good = Sites([(0, 64, [(10, 12, b"T"), (12, 12, b"GG"), (60, 64, b"")]), (8, 40, [])])
    rc = gpu.kset_query_variants_rc(text, *good.args())[0]
    assert rc == abi.HYPO_E_INVALID and b"hypo_gpu_kset_begin" in lib.hypo_gpu_last_error()          # no set, as hypo_gpu_kset_query
    gpu.kset_begin(12, 100)
    try:
        gpu.kset_add(text)
        ok = gpu.kset_query_variants(text, *good.args())
        want = [[qc.seq_stats(v, 12, qc.read_set([text], 12)) for v in vs] for vs in good.strings(text)]
        assert all(g.tolist() == e.tolist() for g, e in zip(ok, expect(want)))
        bad = [[(0, 64, [(12, 14, b"T"), (10, 11, b"G")])],                    # unordered
               [(0, 64, [(10, 14, b"T"), (13, 15, b"G")])],                    # overlapping
               [(0, 40, [(38, 41, b"T")])],                                    # ee > hi
               [(8, 40, [(7, 9, b"T")])],                                      # eb < lo
               [(0, 40, [(12, 11, b"T")])],                                    # ee < eb
               [(0, 65, [])], [(41, 40, [])],                                  # hi > n_bytes, lo > hi
               [(0, 64, [(j, j + 1, b"A") for j in range(13)])],              # 13 edits
               [(8, 40, []), (0, 64, [(2 ** 63, 2 ** 63 + 1, b"A")])]]
        for sites in bad:
            assert gpu.kset_query_variants_rc(text, *Sites(sites).args())[0] == abi.HYPO_E_INVALID, sites
        for field, value in (("ao", 2 ** 40), ("al", 200), ("ao", 2 ** 64 - 1), ("al", 2 ** 32 - 1)):      # ao + al > n_alt_bytes
            s = Sites(good.sites)
            getattr(s, field)[1] = value
            assert gpu.kset_query_variants_rc(text, *s.args())[0] == abi.HYPO_E_INVALID, (field, value)
        s = Sites(good.sites)
        s.eoff[1] = 5; s.eoff[2] = 3                                              # edit_off decreases
        assert gpu.kset_query_variants_rc(text, *s.args())[0] == abi.HYPO_E_INVALID
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        a = good.args()
        mask, out = np.zeros(2, np.uint32), np.zeros(4, np.uint64)
        full = [text, C.c_uint64(64), a[0], C.c_uint64(len(a[0])), p(a[1]), p(a[2]), p(a[3]), C.c_uint32(2), p(a[4]), p(a[5]), p(a[6]), p(a[7]), p(mask), p(out),
                p(out[2:]), None, None]
        assert lib.hypo_gpu_kset_query_variants(*full) == 0
        for i in (0, 2, 4, 5, 6, 8, 9, 10, 11, 12, 13, 14):                       # every required pointer
            args = list(full)
            args[i] = None
            assert lib.hypo_gpu_kset_query_variants(*args) == abi.HYPO_E_INVALID, i
        none = [None, C.c_uint64(0), None, C.c_uint64(0), None, None, None, C.c_uint32(0)] + [None] * 9
        assert lib.hypo_gpu_kset_query_variants(*none) == 0                       # no site: nothing to do
        after = gpu.kset_query_variants(text, *good.args())                       # refused calls change nothing
        assert all(np.array_equal(x, y) for x, y in zip(after, ok))
        assert capi.KSET_MAX_EDITS == 12
    finally:
        gpu.kset_end()
