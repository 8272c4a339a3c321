"""CPU: tests/qv_track_checker.py itself, against brute force on small inputs: every missing window (found by comparing substrings,
as tests/test_qv_checker_cpu.py does) is painted onto a boolean array, the runs of that array are the intervals, and the missing
starts inside a run are counted.  Also the sum rule against qv_checker.seq_stats and a few cases worked out by hand."""
import numpy as np
import pytest

import qv_checker as qc
import qv_track_checker as tc
from test_qv_checker_cpu import COMP, brute_set, rnd


def brute_intervals(seq, k, have):
    """have: the canonical k-mers of the reads as upper-case strings"""
    s = seq.decode() if isinstance(seq, (bytes, bytearray)) else seq
    miss = []
    for i in range(len(s) - k + 1):
        w = s[i:i + k].upper()
        if all(c in "ACGT" for c in w) and min(w, "".join(COMP[c] for c in reversed(w))) not in have:
            miss.append(i)
    covered = np.zeros(len(s) + 1, dtype=bool)                           # (one past the end stays False: every run closes)
    for i in miss:
        covered[i:i + k] = True
    edges = np.flatnonzero(np.diff(np.concatenate([[False], covered]).astype(np.int8)))
    runs = list(zip(edges[0::2].tolist(), edges[1::2].tolist()))
    return [(a, b, sum(a <= i <= b - k for i in miss)) for a, b in runs], miss


def palindrome(k):
    half = "ACGTTGCAAGCTTAGG"[:k // 2]
    return half + "".join(COMP[c] for c in reversed(half))


@pytest.mark.parametrize("k", [12, 21, 22, 31])
def test_against_painting(k):
    rng = np.random.default_rng(300 + k)
    genome = rnd(rng, 3000)
    reads = [genome[p:p + 150] for p in range(0, 2850, 40)] + [rnd(rng, 60, "ACGTN"), rnd(rng, 90).lower(), "A" * 50]
    if k % 2 == 0:
        reads.append(palindrome(k))
    have = brute_set(reads, k)
    R = qc.read_set([r.encode() for r in reads], k)
    mutated = list(genome)
    for p in list(range(7, 3000, 97)) + [0, 1, 2999, 500, 500 + k - 2, 700, 700 + k - 1, 900, 900 + k, 1100, 1100 + k + 1, 1300, 1301, 1302]:
        mutated[p] = "ACGT"[("ACGT".index(mutated[p]) + 1) % 4]
    mutated = "".join(mutated)
    texts = [genome, mutated, mutated.lower(), mutated[:1500] + "N" + mutated[1500:], rnd(rng, 400), rnd(rng, 300, "ACGTN"), rnd(rng, 200, "ACGTacgtn"),
             rnd(rng, k), rnd(rng, k - 1), "", "N" * 50, "A" * 60, "C" * 60, reads[0], rnd(rng, 2 * k), rnd(rng, 2 * k + 1)]
    if k % 2 == 0:
        texts += [palindrome(k), "G" * 30 + palindrome(k).lower() + "T" * 30, palindrome(k)[:-1] + "A"]
    seen = 0
    for t in texts:
        want, miss = brute_intervals(t, k, have)
        assert tc.missing_starts(t, k, R).tolist() == miss, t[:40]
        got = tc.intervals(t, k, R)
        assert got == want, t[:40]
        assert sum(n for _, _, n in got) == qc.seq_stats(t, k, R)[1]
        assert all(b - a >= k for a, b, _ in got) and all(got[j + 1][0] > got[j][1] for j in range(len(got) - 1))
        seen += len(got)
    assert seen > 40
    total, missing, iv_off, st, en, cnt = tc.track([t.encode() for t in texts], k, R)
    assert iv_off[0] == 0 and iv_off[-1] == len(st) == len(en) == len(cnt) == seen
    for s, t in enumerate(texts):
        assert (total[s], missing[s]) == qc.seq_stats(t, k, R)
        assert list(zip(st[iv_off[s]:iv_off[s + 1]], en[iv_off[s]:iv_off[s + 1]], cnt[iv_off[s]:iv_off[s + 1]])) == tc.intervals(t, k, R)
    want_flags = [s % 2 for s in range(len(texts))]
    t2 = tc.track([t.encode() for t in texts], k, R, want_flags)
    assert t2[:2] == (total, missing)
    assert [t2[2][s + 1] - t2[2][s] for s in range(len(texts))] == [(iv_off[s + 1] - iv_off[s]) * want_flags[s] for s in range(len(texts))]


def test_by_hand():
    k = 12
    text = "ACGGTCATTGCAAGCTTAGGCATCGATTACGGCAT"                         # 35 bases, 24 windows
    R = qc.read_set([text.encode()], k)
    assert tc.intervals(text, k, R) == []
    empty = np.zeros(0, np.uint64)
    assert tc.intervals(text, k, empty) == [(0, 35, 24)]
    assert tc.intervals(text[:12], k, empty) == [(0, 12, 1)] and tc.intervals(text[:11], k, empty) == []
    # two windows exactly k apart abut and join; k + 1 apart they do not
    only = lambda starts: qc.read_set([text[a:b + k].encode() for a, b in starts], k)
    assert tc.intervals(text, k, only([(1, 11), (13, 23)])) == [(0, 24, 2)]                  # windows 0 and 12 missing
    assert tc.intervals(text, k, only([(1, 12), (14, 23)])) == [(0, 12, 1), (13, 25, 1)]     # windows 0 and 13 missing
    assert tc.intervals(text, k, only([(0, 22)])) == [(23, 35, 1)]                           # the last window
    assert tc.bed([("c1", text), ("c2", ""), ("c3", text[:20])], k, only([(0, 22)])) == tc.HEADER + "\nc1\t23\t35\t1\n"
    assert tc.parse_bed(tc.HEADER + "\nc1\t23\t35\t1\n") == [("c1", 23, 35, 1)]
