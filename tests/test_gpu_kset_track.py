"""GPU: hypo_gpu_kset_query_track (kset_kernel.hip) against the CPU checker (tests/qv_track_checker.py), as exact integers.

Two kinds of input.  The reads and mutated texts of tests/test_gpu_kset.py, with that file's oddities; and texts with a CHOSEN miss
pattern: for a random text T and a set M of window starts, the reads are the maximal runs of windows outside M, each as a record
T[a : b + k], so that exactly the windows of M are missing (a chosen k-mer may recur elsewhere at k = 12 on longer texts: the wanted
answer is always the checker's, and "the pattern was realised" is asserted only where it holds).  The patterns sit where the
kernels change path: a flag word has 32 positions, a wave's stretch 2048, a workgroup's 8192."""
import ctypes as C

import numpy as np
import pytest

import qv_checker as qc
import qv_track_checker as tc
import test_gpu_kset as tk
from test_gpu_kset import gpu, rnd  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
KS = [12, 21, 22, 31]
EDGES = [32, 2048, 8192]


def reads_for(T, M, k):
    """the records that contain every window of T but those that start in M"""
    n = len(T) - k + 1
    keep = np.ones(n, dtype=bool)
    keep[np.asarray(sorted(M), dtype=np.int64)] = False
    edges = np.flatnonzero(np.diff(np.concatenate([[0], keep.astype(np.int8), [0]])))
    return [T[a:b - 1 + k] for a, b in zip(edges[0::2].tolist(), edges[1::2].tolist())]


def realised(T, M, k, R):
    return tc.missing_starts(T, k, R).tolist() == sorted(M)


def as_lists(out):
    return [np.asarray(x).tolist() for x in out]


def check(gpu, seqs, k, R, want=None):
    """the entry against the checker, against kset_query, and against itself"""
    exp = tc.track(seqs, k, R, want)
    got = as_lists(gpu.kset_query_track(seqs, want=want))
    assert got[2] == exp[2], "iv_off"
    assert got == as_lists(exp)
    assert got[:2] == as_lists(gpu.kset_query(seqs))
    assert as_lists(gpu.kset_query_track(seqs, want=want)) == got
    return got


class Set:
    def __init__(self, gpu, k, recs):
        self.gpu, self.k, self.recs = gpu, k, recs

    def __enter__(self):
        self.gpu.kset_begin(self.k, 1000)
        self.gpu.kset_add(b"\n".join(self.recs))
        return qc.read_set(self.recs, self.k)

    def __exit__(self, *a):
        self.gpu.kset_end()


@pytest.mark.parametrize("k", KS)
def test_reads_and_mutated_texts(gpu, k):
    rng = np.random.default_rng(2000 + k)
    genome, recs = tk.read_records(rng, k)
    qs = tk.queries(rng, k, genome, recs)
    with Set(gpu, k, recs) as R:
        got = check(gpu, qs, k, R)
        assert got[2][-1] > 50 and sum(got[5]) == sum(got[1])
        flags = [s % 2 for s in range(len(qs))]
        for want in (None, [0] * len(qs), flags, [1 - f for f in flags]):
            g = check(gpu, qs, k, R, want)
            assert g[:2] == got[:2]                                       # total and missing do not depend on want
        assert check(gpu, qs, k, R, [0] * len(qs))[2] == [0] * (len(qs) + 1)


@pytest.mark.parametrize("k", KS)
def test_gaps_at_the_edges(gpu, k):
    """two misses k - 2, k - 1, k and k + 1 apart (the first three join, the last does not), the first and the last window of a
    sequence, all of it at positions 31 / 32 / 33, 2047 / 2048 / 2049 and 8191 / 8192 / 8193 of the call"""
    rng = np.random.default_rng(3000 + k)
    L = 8192 + 600
    for gap in (k - 2, k - 1, k, k + 1):
        T = rnd(rng, L)
        M = {0, L - k}
        for e in EDGES:
            M |= {e, e + gap, e + 300, e + 300 + gap}
        recs = reads_for(T, M, k)
        with Set(gpu, k, recs) as R:
            assert realised(T, M, k, R) or k == 12
            for shift in (-1, 0, 1):
                # a first sequence without a window moves T: its position 32 + shift ... is the call's 64, 2080, 8224: a word's edge; 2048 + 32, ...: a wave's; ...
                for lead in (b"", b"N" * (32 + shift), b"N" * (2048 + shift), b"N" * (8192 + shift), rnd(rng, k - 1) + b"N" * (8192 - k + 1 + shift)):
                    seqs = [lead, T]
                    got = check(gpu, seqs, k, R)
                    if realised(T, M, k, R):
                        ivs = list(zip(got[3], got[4], got[5]))
                        for e in EDGES:
                            joined = (e, e + gap + k, 2) in ivs
                            assert joined == (gap <= k), (gap, e, ivs)
                            assert joined or ((e, e + k, 1) in ivs and (e + gap, e + gap + k, 1) in ivs)
                        assert ivs[0] == (0, k, 1) and ivs[-1] == (L - k, L, 1)


@pytest.mark.parametrize("k", KS)
def test_one_long_interval_among_short_ones(gpu, k):
    """an interval of about 3 x 8192 windows: it spans several workgroups and its count needs the scanned sums"""
    rng = np.random.default_rng(4000 + k)
    n_long = 3 * 8192 + 77
    L = 3000 + n_long + 3000
    T = rnd(rng, L)
    M = set(range(3000, 3000 + n_long)) | set(range(10, 2900, 131)) | set(range(3000 + n_long + 50, L - k, 97)) | {500, 501, 502}
    recs = reads_for(T, M, k)
    with Set(gpu, k, recs) as R:
        for lead in (b"", b"N" * 31, rnd(rng, 5000)):
            got = check(gpu, [lead, T, T[2990:3000 + n_long + 40]], k, R)
        if realised(T, M, k, R):
            at = got[2][1]
            ivs = list(zip(got[3][at:], got[4][at:], got[5][at:]))
            assert (3000, 3000 + n_long - 1 + k, n_long) in ivs
        # every window missing, and none
        nothing, everything = recs[0], rnd(rng, 2 * 8192 + 5)
        got = check(gpu, [nothing, everything, nothing, b"", everything[:k], everything[:k - 1]], k, R)
        n_all = len(everything) - k + 1
        if qc.seq_stats(everything, k, R)[1] == n_all:
            assert got[2] == [0, 0, 1, 1, 1, 2, 2] and (got[3], got[4], got[5]) == ([0, 0], [len(everything), k], [n_all, 1])


@pytest.mark.parametrize("k", KS)
def test_sequence_sets(gpu, k):
    rng = np.random.default_rng(5000 + k)
    genome = rnd(rng, 12000)
    recs = [genome[p:p + 200] for p in range(0, 11800, 50)]
    mutated = tk.mutate(rng, genome, 0.004)
    other = rnd(rng, 12000)                                               # every window missing (at k = 12: nearly every)
    with Set(gpu, k, recs) as R:
        assert as_lists(gpu.kset_query_track([])) == [[], [], [0], [], [], []]
        for seqs in ([mutated], [b""], [b"", b""], [b"", mutated[:k - 1], b"", mutated, b"", b""], [mutated[:k - 1]] * 5, [mutated[:k]], [b"N" * 100]):
            check(gpu, seqs, k, R)
        # sequence ends at 32 / 2048 / 8192 - 1, + 0, + 1 of the call; with `other` every end is book-ended by two missing windows
        for text in (mutated, other):
            for shift in (-1, 0, 1):
                cuts = [0, 32 + shift, 2048 + shift, 8192 + shift, len(text)]
                seqs = [text[a:b] for a, b in zip(cuts, cuts[1:])]
                got = check(gpu, seqs, k, R)
                if text is other and qc.seq_stats(other, k, R)[1] == len(other) - k + 1:
                    assert got[2] == [0, 1, 2, 3, 4] and got[3] == [0] * 4 and got[4] == [len(s) for s in seqs]
        # forty back-to-back sequences of exactly k bases, all missing: forty intervals [0, k), several sequence starts in a flag word
        forty = [other[i * k:(i + 1) * k] for i in range(40)]
        got = check(gpu, forty, k, R)
        if sum(got[1]) == 40:
            assert got[2] == list(range(41)) and got[3] == [0] * 40 and got[4] == [k] * 40 and got[5] == [1] * 40
        check(gpu, [b"N" * 17] + forty + [mutated[:100]] + forty[:3], k, R, [s % 2 for s in range(45)])
    # the book-ended pair across a sequence end: the last window of one sequence and the first of the next, and nothing else
    A, B = rnd(rng, 700), rnd(rng, 300)
    pair_recs = reads_for(A, {len(A) - k}, k) + reads_for(B, {0}, k)
    with Set(gpu, k, pair_recs) as R:
        for lead in (0, 32 - 700 % 32, 8192 - 700):
            got = check(gpu, [b"N" * lead, A, B], k, R)
            if realised(A, {len(A) - k}, k, R) and realised(B, {0}, k, R):
                assert got[2:] == [[0, 0, 1, 2], [len(A) - k, 0], [len(A), k], [1, 1]]


def test_room_counting_call_and_argument_errors(gpu):
    from hypo_amd import abi
    k = 21
    rng = np.random.default_rng(6)
    genome = rnd(rng, 9000)
    seqs = [tk.mutate(rng, genome, 0.003), b"", tk.mutate(rng, genome[:3000], 0.01)]
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    lib = gpu.lib
    off = np.array([0, 40], dtype=np.uint64)
    two, iv_off = np.full(2, 5, np.uint64), np.full(2, 5, np.uint64)
    assert lib.hypo_gpu_kset_query_track(b"ACGT" * 10, p(off), C.c_uint32(1), None, p(two), p(two[1:]), p(iv_off), None, None, None, C.c_uint64(0)) == abi.HYPO_E_INVALID
    assert b"hypo_gpu_kset_begin" in lib.hypo_gpu_last_error()          # no set
    assert two.tolist() == [5, 5] and iv_off.tolist() == [5, 5]
    with Set(gpu, k, [genome]) as R:
        exp = as_lists(tc.track(seqs, k, R))
        n_iv = exp[2][-1]
        assert n_iv > 10
        good = as_lists(gpu.kset_query_track(seqs))
        assert good == exp
        # the counting call, and room one short: HYPO_E_WORKSPACE, iv_off right, the arrays untouched
        for cap in (0, n_iv - 1):
            out = gpu.kset_query_track_rc(seqs, iv_cap=cap)
            assert out[0] == abi.HYPO_E_WORKSPACE
            assert as_lists(out[1:4]) == exp[:3]
            assert all(a.tolist() == [abi.TRACK_UNTOUCHED] * cap for a in out[4:])
        out = gpu.kset_query_track_rc(seqs, iv_cap=n_iv + 3)             # more room than needed: the rest stays untouched
        assert out[0] == 0 and [a[:n_iv].tolist() for a in out[4:]] == exp[3:] and all(a[n_iv:].tolist() == [abi.TRACK_UNTOUCHED] * 3 for a in out[4:])
        assert gpu.kset_query_track_rc([genome, genome[:500]], iv_cap=0)[0] == 0                       # no interval: the counting call succeeds
        assert gpu.kset_query_track_rc(seqs, want=[0, 0, 0], iv_cap=0)[0] == 0
        # refused calls change nothing
        text = b"".join(seqs)
        offs = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
        bad = offs.copy(); bad[1], bad[2] = bad[2] + 1, bad[1]
        mk = lambda n: np.full(n, 9, np.uint64)
        for args in ((bad, mk(3), mk(3), mk(4), mk(n_iv), mk(n_iv), mk(n_iv), n_iv),               # off[] decreases
                     (None, mk(3), mk(3), mk(4), mk(n_iv), mk(n_iv), mk(n_iv), n_iv),              # required pointers
                     (offs, None, mk(3), mk(4), mk(n_iv), mk(n_iv), mk(n_iv), n_iv),
                     (offs, mk(3), None, mk(4), mk(n_iv), mk(n_iv), mk(n_iv), n_iv),
                     (offs, mk(3), mk(3), None, mk(n_iv), mk(n_iv), mk(n_iv), n_iv),
                     (offs, mk(3), mk(3), mk(4), None, mk(n_iv), mk(n_iv), n_iv),
                     (offs, mk(3), mk(3), mk(4), mk(n_iv), None, mk(n_iv), n_iv),
                     (offs, mk(3), mk(3), mk(4), mk(n_iv), mk(n_iv), None, n_iv)):
            ptrs = [None if a is None else p(a) for a in args[:7]]
            rc = lib.hypo_gpu_kset_query_track(text, ptrs[0], C.c_uint32(3), None, *ptrs[1:], C.c_uint64(args[7]))
            assert rc == abi.HYPO_E_INVALID, args
            assert all(a is None or a is bad or a is offs or set(a.tolist()) == {9} for a in args[:7])
        assert lib.hypo_gpu_kset_query_track(None, p(offs), C.c_uint32(3), None, p(mk(3)), p(mk(3)), p(mk(4)), None, None, None, C.c_uint64(0)) == abi.HYPO_E_INVALID
        assert as_lists(gpu.kset_query_track(seqs)) == good               # a valid call afterwards is unchanged
        assert as_lists(gpu.kset_query_track(text, offs)) == good         # one text with its offsets
    assert lib.hypo_gpu_kset_end() == 0
