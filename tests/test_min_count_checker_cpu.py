"""CPU: tests/min_count_checker.py against a brute-force dictionary count, and its threshold rule on hand-made histograms."""
import numpy as np
import pytest

import min_count_checker as mc
import qv_checker as qc

COMP = bytes.maketrans(b"ACGT", b"TGCA")
CODE = {ord(c): i for i, c in enumerate("ACGT")}


def brute(recs, k):
    """{canonical code: windows} by walking every window of every record as a Python string"""
    d = {}
    for r in recs:
        r = r.upper()
        for i in range(len(r) - k + 1):
            w = r[i:i + k]
            if any(c not in CODE for c in w):
                continue
            f = sum(CODE[c] << (2 * (k - 1 - j)) for j, c in enumerate(w))
            rc = sum(CODE[c] << (2 * (k - 1 - j)) for j, c in enumerate(w.translate(COMP)[::-1]))
            d[min(f, rc)] = d.get(min(f, rc), 0) + 1
    return d


def palindrome(k):
    half = b"ACGTTGCAAGCTTAGG"[:k // 2]
    return half + half.translate(COMP)[::-1]


@pytest.mark.parametrize("k", [12, 13, 22, 31])
def test_counts_and_reliable_sets_equal_brute_force(k):
    rng = np.random.default_rng(700 + k)
    rnd = lambda n, alphabet=b"ACGT": bytes(rng.choice(list(alphabet), n).astype(np.uint8))
    genome = rnd(300)
    recs = []
    for _ in range(60):                                                     # 30 reads of each strand, so counts of 1 to about 20
        p = int(rng.integers(0, 200))
        r = genome[p:p + 100]
        recs.append(r.translate(COMP)[::-1] if rng.random() < 0.5 else r)
    recs += [rnd(80, b"ACGTN"), rnd(80).lower(), rnd(60, b"ACGTacgtnR"), b"", rnd(k - 1), rnd(k - 1) + b"N" + rnd(k - 1)]
    recs += [b"A" * (k + 299)]                                              # one key 300 times: it stops at 255
    if k % 2 == 0:
        recs += [palindrome(k), b"G" * 3 + palindrome(k).lower() + b"T" * 3, palindrome(k)]
    want = brute(recs, k)
    keys, counts = mc.read_counts(recs, k)
    assert keys.tolist() == sorted(want) and keys.dtype == np.uint64
    assert counts.tolist() == [min(want[x], 255) for x in sorted(want)]
    assert counts.max() == 255 and want[0] == 300 and counts.min() == 1
    if k % 2 == 0:
        pal = int(qc.canonical_windows(palindrome(k), k)[0])
        assert want[pal] == 3                                               # a palindromic window counts once, not once per strand
    assert np.array_equal(keys, qc.read_set(recs, k))                       # R_1 is R
    h = mc.histogram(counts)
    assert h.shape == (256,) and h[0] == 0 and h.sum() == keys.size and h[255] == 1
    for t in (1, 2, 3, 7, 255):
        Rt = mc.reliable_set(keys, counts, t)
        assert Rt.tolist() == [x for x in sorted(want) if min(want[x], 255) >= t]
        assert Rt.size == h[t:].sum()
    assert mc.reliable_set(keys, counts, 1).size > mc.reliable_set(keys, counts, 2).size > mc.reliable_set(keys, counts, 255).size == 1
    # the existing checkers take R_t where they take R
    q = genome[:150]
    assert qc.seq_stats(q, k, mc.reliable_set(keys, counts, 255))[1] == 150 - k + 1
    assert qc.seq_stats(b"a" * 40, k, mc.reliable_set(keys, counts, 255)) == (40 - k + 1, 0)


def hist(pairs, fill=0):
    h = np.full(256, fill, np.int64)
    h[0] = 0
    for c, v in pairs:
        h[c] = v
    return h


def test_threshold_rule():
    falling = np.arange(1000, 1000 - 256, -1)                               # never stops falling: no valley
    assert mc.threshold(falling, "valley") == 2
    assert mc.threshold(np.zeros(256, np.int64), "valley") == 2             # h[2] <= h[3] at once
    assert mc.threshold(hist([(1, 900), (2, 50), (3, 10), (4, 4), (5, 9), (6, 30)]), "valley") == 4
    assert mc.threshold(hist([(1, 900), (2, 50), (3, 10), (4, 10), (5, 3)], fill=0), "valley") == 3       # a plateau counts as the valley
    assert mc.threshold(hist([(1, 900), (2, 50), (3, 60)]), "valley") == 2
    h = np.arange(2000, 2000 - 256, -1)                                      # falling until 254, then up: the last c the rule looks at
    h[255] = h[254]
    assert mc.threshold(h, "valley") == 254
    h[255] = h[254] - 1
    assert mc.threshold(h, "valley") == 2
    h = hist([(1, 5), (2, 9)])                                              # h[1] is never looked at
    h[1] = 0
    assert mc.threshold(h, "valley") == 3
    for t in (1, 2, 7, 255):
        assert mc.threshold(falling, t) == t and mc.threshold(falling, str(t)) == t
    for bad in (0, 256):
        with pytest.raises(AssertionError):
            mc.threshold(falling, bad)


def test_info_line():
    h = hist([(1, 900), (2, 50), (3, 10), (4, 4), (5, 9), (6, 30), (255, 1)])
    assert mc.info_line(21, h, "valley") == "[Hypo::Hypo] Info: k-mer min count (k = 21): >= 4 (valley), 44 of 1004 read k-mers reliable"
    assert mc.info_line(16, h, 2) == "[Hypo::Hypo] Info: k-mer min count (k = 16): >= 2 (given), 104 of 1004 read k-mers reliable"
