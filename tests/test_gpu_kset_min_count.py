"""GPU: hypo_gpu_kset_min_count (kset_kernel.hip, the kset_*_min_kernel variants of the four query kernels) against the CPU checkers
called with R_t = the k-mers the reads have at least t times (tests/min_count_checker.py), as exact integers.

The reads are those of tests/test_gpu_kset.py (a 20 kbp genome at 30x with 1 % error: most distinct k-mers are errors seen once, the
genome's own are seen about 25 times) and one read of 400 A, so that one key stops at 255.  A threshold that bites nowhere would pass
nothing here: every k asserts that the valley is at least 3, that more is missing at t = 2 than at t = 1, and that at least 100 of the
216 queries answer differently at the valley."""
import functools

import numpy as np
import pytest

import min_count_checker as mc
import qv_checker as qc
import qv_track_checker as tc
import test_gpu_kset as tk
from test_gpu_kset_spans import case as span_case, group, piece  # noqa: F401  (the fixtures)
from test_gpu_kset_variants import expect, site_sets

pytestmark = pytest.mark.gpu
KS = [12, 21, 22, 31]
GROUPS = [32, 64]


@pytest.fixture(scope="module")
def gpu():
    from hypo_amd import capi
    return capi.HypoGpu(0)


class Case:
    """reads, queries and the checker's answers of one k, built once and never changed"""

    def __init__(self, k):
        rng = np.random.default_rng(2000 + k)
        self.k = k
        self.genome, recs = tk.read_records(rng, k)
        self.qs = tk.queries(rng, k, self.genome, recs)
        self.recs = recs + [b"A" * 400]
        self.blob = b"\n".join(self.recs)
        self.keys, self.counts = mc.read_counts(self.recs, k)
        self.h = mc.histogram(self.counts)
        self.valley = mc.threshold(self.h, "valley")
        self._want = {}
        assert self.counts.max() == 255 and self.h[255] == 1
        assert self.valley >= 3
        m1, m2 = (sum(m for _, m in self.want(t)) for t in (1, 2))
        assert m2 > m1
        assert sum(a != b for a, b in zip(self.want(1), self.want(self.valley))) >= 100

    def R(self, t):
        return mc.reliable_set(self.keys, self.counts, t)

    def want(self, t):
        if t not in self._want:
            self._want[t] = [qc.seq_stats(q, self.k, self.R(t)) for q in self.qs]
        return self._want[t]


@functools.lru_cache(maxsize=None)
def case(k):
    return Case(k)


def pairs(out):
    return [(int(t), int(m)) for t, m in zip(*out)]


class Counting:
    """a set that counts, filled with `adds`"""

    def __init__(self, gpu, k, expected, adds=(), n_texts=1):
        self.gpu, self.k, self.expected, self.adds, self.n_texts = gpu, k, expected, adds, n_texts

    def __enter__(self):
        self.gpu.kset_begin(self.k, self.expected)
        self.gpu.kset_counts_enable(self.n_texts)
        for a in self.adds:
            self.gpu.kset_add(a)
        return self.gpu

    def __exit__(self, *a):
        self.gpu.kset_end()


@pytest.mark.parametrize("k", KS)
def test_query_at_every_threshold(gpu, k):
    from hypo_amd import abi
    c = case(k)
    inv = abi.HYPO_E_INVALID
    assert gpu.kset_min_count_rc(2) == inv and b"hypo_gpu_kset_begin" in gpu.lib.hypo_gpu_last_error()        # no set
    gpu.kset_begin(k, c.keys.size)
    try:
        gpu.kset_add(c.blob)
        plain = pairs(gpu.kset_query(c.qs))                                  # a set that does not count: presence
        assert gpu.kset_min_count_rc(2) == inv and b"hypo_gpu_kset_counts_enable" in gpu.lib.hypo_gpu_last_error()
        assert pairs(gpu.kset_query(c.qs)) == plain
    finally:
        gpu.kset_end()
    assert plain == c.want(1)
    with Counting(gpu, k, c.keys.size, [c.blob]):
        assert gpu.kset_size()[0] == c.keys.size
        assert pairs(gpu.kset_query(c.qs)) == plain                          # hypo_gpu_kset_begin starts at t = 1
        for t in (1, 2, c.valley, 255, 1):
            gpu.kset_min_count(t)
            assert pairs(gpu.kset_query(c.qs)) == c.want(t), t
            assert (t == 1) == (c.want(t) == plain)
        gpu.kset_min_count(255)
        got = pairs(gpu.kset_query([b"A" * 100, c.genome, b"a" * (k - 1), b"T" * k]))
        assert got == [qc.seq_stats(s, k, c.R(255)) for s in (b"A" * 100, c.genome, b"a" * (k - 1), b"T" * k)]
        assert got[0] == (100 - k + 1, 0) and got[3] == (1, 0) and got[1][1] >= got[1][0] - 2 and got[1][0] == len(c.genome) - k + 1
        # refused calls change nothing
        gpu.kset_min_count(c.valley)
        for t in (0, 256, 2 ** 31, 2 ** 32 - 1):
            assert gpu.kset_min_count_rc(t) == inv and b"1..255" in gpu.lib.hypo_gpu_last_error()
        assert pairs(gpu.kset_query(c.qs)) == c.want(c.valley)
        # the other entry points do not know of t
        assert gpu.kset_size()[0] == c.keys.size
        assert gpu.kset_spectrum(0)[:, 0].astype(np.int64).tolist() == c.h.tolist()
        assert gpu.kset_mark(0, [c.genome]) == qc.seq_stats(c.genome, k, c.keys)
        gpu.kset_min_count(2)                                                # after a mark, too: it does not close or open anything
        assert pairs(gpu.kset_query(c.qs)) == c.want(2)
    # the next set starts at 1 again
    with Counting(gpu, k, c.keys.size, [c.blob]):
        assert pairs(gpu.kset_query(c.qs)) == plain


@pytest.mark.parametrize("k", KS)
def test_counts_move_with_their_keys(gpu, k):
    """the same bytes in 4099-byte adds that overlap by exactly k - 1, into the smallest table: it grows, the answers are the same"""
    c = case(k)
    with Counting(gpu, k, 1):
        sizes, chunk, at = [gpu.kset_size()[1]], 4099, 0
        while True:
            gpu.kset_add(c.blob[at:at + chunk])
            tb = gpu.kset_size()[1]
            if tb != sizes[-1]:
                sizes.append(tb)
            if at + chunk >= len(c.blob):
                break
            at += chunk - (k - 1)
        assert len(sizes) >= 4 and sizes == sorted(sizes), sizes          # grew at least three times
        assert gpu.kset_size()[0] == c.keys.size
        for t in (2, c.valley):
            gpu.kset_min_count(t)
            assert pairs(gpu.kset_query(c.qs)) == c.want(t), t


@pytest.mark.parametrize("k", KS)
def test_threshold_is_applied_when_the_query_runs(gpu, k):
    """t is set on the empty set, then half of the reads, a query, the other half, a query: each sees the counts of its moment"""
    c = case(k)
    half = len(c.recs) // 2
    first = b"\n".join(c.recs[:half])
    keys1, counts1 = mc.read_counts(c.recs[:half], k)
    R1 = mc.reliable_set(keys1, counts1, 2)
    qs = c.qs[:40]
    with Counting(gpu, k, 1):
        gpu.kset_min_count(2)
        assert pairs(gpu.kset_query(qs)) == [(t, t) for t, _ in c.want(1)[:40]]           # the empty set: every window is missing
        gpu.kset_add(first)
        got = pairs(gpu.kset_query(qs))
        assert got == [qc.seq_stats(q, k, R1) for q in qs] and got != c.want(2)[:40]
        gpu.kset_add(b"\n".join(c.recs[half:]))                             # the table grows under the threshold: it stays
        assert pairs(gpu.kset_query(qs)) == c.want(2)[:40]


@pytest.mark.parametrize("k", KS)
def test_staging_seams(gpu, k):
    """the shapes of test_gpu_kset_counts.test_staging_seams as the text: sequences that end 5 bytes before, exactly at and just after
    a multiple of the 8192 bytes a workgroup stages, and a window that starts in the last byte of a lane's 32-byte stretch.  The
    reads hold every sequence, every second one twice: at t = 2 those lack nothing and the others nearly everything."""
    rng = np.random.default_rng(3000 + k)
    ends = [8192 - 5, 2 * 8192, 3 * 8192 + 1]
    seqs, at = [], 0
    for e in ends:
        seqs.append(tk.rnd(rng, e - at))
        at = e
    lone = tk.rnd(rng, k)                                                  # its only window starts at a position = 31 mod 32
    seqs.append(b"N" * ((31 - at) % 32) + lone + b"N" * 3)
    seqs.append(tk.rnd(rng, 100))
    assert (sum(len(s) for s in seqs[:3]) + seqs[3].index(lone)) % 32 == 31
    reads = seqs + seqs[::2]
    keys, counts = mc.read_counts(reads, k)
    with Counting(gpu, k, 1000, [b"\n".join(reads)]):
        for t in (1, 2, 3):
            gpu.kset_min_count(t)
            want = [qc.seq_stats(s, k, mc.reliable_set(keys, counts, t)) for s in seqs]
            assert pairs(gpu.kset_query(seqs)) == want, t
            trk = [np.asarray(x).tolist() for x in gpu.kset_query_track(seqs)]
            assert trk == [list(x) for x in tc.track(seqs, k, mc.reliable_set(keys, counts, t))], t
            if t == 2:
                assert [m for _, m in want][::2] == [0, 0, 0] and want[3] == (1, 1) and want[1][1] >= 0.95 * want[1][0]      # (k = 12: a few chance hits)
            if t == 3:
                assert all(m >= 0.95 * tot for tot, m in want)                           # (k = 12: 2 of the 89 windows of the last one are chance hits)


# ---- spans and variants: the texts, spans and sites of tests/test_gpu_kset_spans.py and tests/test_gpu_kset_variants.py ---------
@functools.lru_cache(maxsize=None)
def span_refs(k, piece):
    """(keys, counts, valley, ref) for the reads of test_gpu_kset_spans.case: ref(t, bytes) = the checker's pair against R_t"""
    blob = span_case(k, piece)[0]
    keys, counts = mc.read_counts(blob, k)
    valley = mc.threshold(mc.histogram(counts), "valley")
    assert valley >= 3
    Rs, memo = {}, {}

    def ref(t, s):
        if t not in Rs:
            Rs[t] = mc.reliable_set(keys, counts, t)
        if (t, s) not in memo:
            memo[(t, s)] = qc.seq_stats(s, k, Rs[t])
        return memo[(t, s)]
    return keys, counts, valley, ref


@pytest.mark.parametrize("group", GROUPS, indirect=True)
@pytest.mark.parametrize("k", KS)
def test_spans(gpu, piece, k, group):
    blob, R, text, sets, want1 = span_case(k, piece)
    keys, counts, valley, ref = span_refs(k, piece)
    assert np.array_equal(keys, R)
    with Counting(gpu, k, keys.size, [blob]):
        differ = 0
        for t in (2, valley):
            gpu.kset_min_count(t)
            for name, lo, hi in sets:
                if name == "edge shuffled":
                    continue
                total, missing = gpu.kset_query_spans(text, lo, hi)
                want = [ref(t, text[int(a):int(b)]) for a, b in zip(lo, hi)]
                got = list(zip(total.tolist(), missing.tolist()))
                bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
                assert not bad, (t, name, [(int(lo[i]), int(hi[i]), got[i], want[i]) for i in bad[:5]])
                differ += int(np.count_nonzero(missing != want1[name][1]))
        assert differ >= 100
        gpu.kset_min_count(1)
        name, lo, hi = sets[0]
        total, missing = gpu.kset_query_spans(text, lo, hi)
        assert np.array_equal(total, want1[name][0]) and np.array_equal(missing, want1[name][1])


@pytest.mark.parametrize("group", GROUPS, indirect=True)
@pytest.mark.parametrize("k", KS)
def test_variants(gpu, piece, k, group):
    blob, R, text, _, _ = span_case(k, piece)
    keys, counts, valley, ref = span_refs(k, piece)
    sets = site_sets(k, piece)
    with Counting(gpu, k, keys.size, [blob]):
        masks_differ = 0
        for t in (2, valley):
            gpu.kset_min_count(t)
            for name in ("edge", "one long among short", "plain"):
                S, want1 = sets[name]
                exp = expect([[ref(t, v) for v in vs] for vs in S.strings(text)])
                got = gpu.kset_query_variants(text, *S.args())
                for what, g, e in zip(("best_mask", "best_total", "best_missing", "var_total", "var_missing"), got, exp):
                    bad = np.flatnonzero(g != e)
                    assert g.shape == e.shape and bad.size == 0, (t, name, what, [(int(i), int(g[i]), int(e[i])) for i in bad[:5]])
                nov = gpu.kset_query_variants(text, *S.args(), variants=False)               # var_* NULL: the same best_*
                assert all(np.array_equal(a, b) for a, b in zip(nov[:3], got[:3]))
                masks_differ += int(np.count_nonzero(got[0] != expect(want1)[0]))
        assert masks_differ >= 1
        gpu.kset_min_count(1)
        S, want1 = sets["edge"]
        assert all(np.array_equal(g, e) for g, e in zip(gpu.kset_query_variants(text, *S.args()), expect(want1)))


# ---- the track -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_track(gpu, k):
    from hypo_amd import abi
    c = case(k)
    flags = [s % 2 for s in range(len(c.qs))]
    with Counting(gpu, k, c.keys.size, [c.blob]):
        n_iv = {}
        for t in (2, c.valley):
            gpu.kset_min_count(t)
            R = c.R(t)
            for want in (None, flags):
                exp = [list(x) for x in tc.track(c.qs, k, R, want)]
                got = [np.asarray(x).tolist() for x in gpu.kset_query_track(c.qs, want=want)]
                assert got[2] == exp[2], (t, "iv_off")
                assert got == exp, t
                assert list(zip(got[0], got[1])) == c.want(t)                   # total and missing do not depend on want
            assert sum(got[5]) == sum(m for (_, m), f in zip(c.want(t), flags) if f)
            # the counting call: no room, no arrays, the number of intervals
            exp = tc.track(c.qs, k, R)
            out = gpu.kset_query_track_rc(c.qs, iv_cap=0)
            assert out[0] == abi.HYPO_E_WORKSPACE and out[3].tolist() == list(exp[2]) and list(zip(out[1].tolist(), out[2].tolist())) == c.want(t)
            n_iv[t] = int(out[3][-1])
        gpu.kset_min_count(1)
        got1 = [np.asarray(x).tolist() for x in gpu.kset_query_track(c.qs)]
        assert got1 == [list(x) for x in tc.track(c.qs, k, c.keys)]
        assert sum(got1[1]) < sum(m for _, m in c.want(2))
