"""CPU: tests/guard_checker.py (the contract of `hypo --kmer-guard`) against brute force.  Over every subset of a contig's
clusters the guard's choice has the fewest missing k-mers and, among the subsets with as few, accepts the most; the missing count
of every subset is the draft's plus the sum of (a_c - r_c) over the subset (no window touches two clusters), hence
missing(final) <= min(missing(D), missing(P)).  Small k (4..6) keeps random texts full of hits and misses."""
import itertools

import numpy as np
import pytest

import edit_checker as ec
import guard_checker as gc
import qv_checker as qc


def rnd(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(list(alphabet), n))


def other(rng, base):
    return rng.choice([c for c in "ACGT" if c != base])


def random_records(rng, D, k, start=None, max_clusters=6):
    """non-overlapping records in draft order: substitutions, padded insertions and deletions, gaps around k - 1"""
    recs, p = [], int(rng.integers(0, k + 2)) if start is None else start
    while p + 4 < len(D):
        kind = rng.integers(3)
        if kind == 0:
            n = int(rng.integers(1, 3))
            ref = D[p:p + n]
            alt = "".join(other(rng, c) for c in ref)
        elif kind == 1:
            ref = D[p]
            alt = ref + rnd(rng, int(rng.integers(1, 4)))
        else:
            ref = D[p:p + 1 + int(rng.integers(1, 3))]
            alt = ref[0]
        recs.append((p + 1, ref, alt, "."))
        if len(gc.clusters(recs, k)) > max_clusters:
            recs.pop()
            break
        p += len(ref) + int(rng.choice([0, 1, k - 2, k - 1, k, k + 3, 2 * k]))
    return recs


def random_set(rng, D, P, k):
    """k-mers of random stretches of D and of P, and a few random ones"""
    parts = []
    for text in (D, P):
        for _ in range(int(rng.integers(0, 6))):
            a = int(rng.integers(0, max(1, len(text) - k)))
            parts.append(text[a:a + int(rng.integers(k, 4 * k))].encode())
    parts.append(rnd(rng, 3 * k).encode())
    return qc.read_set(parts, k)


def check_against_brute_force(D, recs, k, R):
    res = gc.guard(D, recs, k, R)
    cl = res.clusters
    assert len(cl) <= 6
    P = ec.apply(recs, D)
    mD, mP = gc.missing(D, k, R), gc.missing(P, k, R)
    accepted = tuple(a <= r for r, a in res.scores)
    by_subset = {}
    for pick in itertools.product((False, True), repeat=len(cl)):
        sub = [r for c, on in zip(cl, pick) if on for r in recs[c[0]:c[1]]]
        m = gc.missing(ec.apply(sub, D), k, R)
        by_subset[pick] = m
        assert m == mD + sum(a - r for (r, a), on in zip(res.scores, pick) if on)       # the identity, for every subset
    best = min(by_subset.values())
    assert by_subset[accepted] == best == gc.missing(res.text, k, R)
    minima = [p for p, m in by_subset.items() if m == best]
    assert all(sum(p) < sum(accepted) or p == accepted for p in minima)                  # among minima it accepts the most
    assert res.text == ec.apply([r for c, on in zip(cl, accepted) if on for r in recs[c[0]:c[1]]], D)
    assert res.filters == [("PASS" if on else "kmer") for c, on in zip(cl, accepted) for _ in range(c[0], c[1])]
    assert best <= min(mD, mP)                                                            # the inequality
    assert by_subset[(True,) * len(cl)] == mP and by_subset[(False,) * len(cl)] == mD
    assert (res.n_clusters, res.n_records) == (len(cl), len(recs))
    assert (res.rej_clusters, res.rej_records) == (accepted.count(False), res.filters.count("kmer"))
    return res


@pytest.mark.parametrize("k", [4, 5, 6])
def test_random_contigs(k):
    rng = np.random.default_rng(100 + k)
    seen_reject = seen_tie = seen_multi = 0
    for _ in range(60):
        D = rnd(rng, int(rng.integers(30, 90)), "ACGT" * 6 + "N")
        recs = random_records(rng, D, k)
        if not recs:
            continue
        R = random_set(rng, D, ec.apply(recs, D), k)
        res = check_against_brute_force(D, recs, k, R)
        seen_reject += res.rej_clusters > 0
        seen_tie += any(a == r for r, a in res.scores)
        seen_multi += any(c[1] - c[0] > 1 for c in res.clusters)
    assert seen_reject > 5 and seen_tie > 5 and seen_multi > 5


@pytest.mark.parametrize("k", [4, 5, 6, 21])
def test_cluster_rule_at_the_gap(k):
    """k - 2 unchanged bases between two records: one length-k window holds both edits, one cluster; k - 1 or k: two"""
    rng = np.random.default_rng(k)
    D = rnd(rng, 4 * k + 20)
    for gap, want in ((k - 2, 1), (k - 1, 2), (k, 2)):
        p = k + 3
        q = p + 1 + gap
        recs = [(p + 1, D[p], other(rng, D[p]), "."), (q + 1, D[q], other(rng, D[q]), ".")]
        cl = gc.clusters(recs, k)
        assert len(cl) == want, (gap, cl)
        if want == 1:
            assert cl == [(0, 2, p, q + 1, p, q + 1)]
        else:
            assert cl == [(0, 1, p, p + 1, p, p + 1), (1, 2, q, q + 1, q, q + 1)]
        R = qc.read_set([D.encode()], k)
        res = check_against_brute_force(D, recs, k, R)
        assert res.filters == ["kmer", "kmer"] and res.text == D     # every draft k-mer is in R, the edits only add strangers


def test_polished_span_follows_the_length_changes():
    k = 5
    D = "ACGTTGCAAGGCTTACCGATAGGCTAGCTTAACG"
    recs = [(3, "G", "GTT", "."), (20, "TAG", "T", "."), (22 + k, "G", "C", ".")]          # gap 20+2 -> 22+k-1: k - 1 bases, a new cluster
    assert D[2] == "G" and D[19:22] == "TAG" and D[21 + k] == "G"
    assert gc.clusters(recs, k) == [(0, 1, 2, 3, 2, 5), (1, 2, 19, 22, 21, 22), (2, 3, 21 + k, 22 + k, 21 + k, 22 + k)]
    P = ec.apply(recs, D)
    for c in gc.clusters(recs, k):
        ref, alt = gc.spans(D, P, c, k)
        n = min(k - 1, c[2])
        assert ref[:n] == alt[:n] and ref[-(k - 1):] == alt[-(k - 1):]                     # the flanks are the same bytes


@pytest.mark.parametrize("k", [4, 6])
def test_clusters_at_the_contig_ends(k):
    rng = np.random.default_rng(7 * k)
    for _ in range(20):
        D = rnd(rng, 40)
        first = int(rng.integers(0, k - 1))
        last = len(D) - 1 - int(rng.integers(0, k - 1))
        recs = [(first + 1, D[first], other(rng, D[first]), "."), (last + 1, D[last], other(rng, D[last]), ".")]
        if first == 0:
            recs[0] = (1, D[0], rnd(rng, 2) + D[0], ".")                                  # an insertion before the first base
        P = ec.apply(recs, D)
        cl = gc.clusters(recs, k)
        assert len(cl) == 2
        ref, alt = gc.spans(D, P, cl[0], k)
        assert ref == D[:first + 1 + k - 1] and alt == P[:cl[0][5] + k - 1]
        ref, alt = gc.spans(D, P, cl[1], k)
        assert ref == D[last - k + 1:] and alt == P[cl[1][4] - k + 1:]
        check_against_brute_force(D, recs, k, random_set(rng, D, P, k))


def test_padded_indels_n_and_the_merged_first_record():
    """records as edit_checker.records builds them from unit scripts: padded insertions and deletions, an N of the draft next to an
    edit, and the record at position 1 that merges an insertion before the first base with a deletion after it"""
    k = 5
    rng = np.random.default_rng(3)
    D = "ACGTNACGGATTACAGGCTTNCATCGGATCCGATAGCTAGGCTTAACCGGT"
    units = [(0, 2, "TT" + D[0], [(2, "I"), (1, "="), (1, "D")]),                          # I2 =1 D1 at 0: one merged record
             (5, 9, "A" + "GGG" + D[6:9], [(1, "="), (3, "I"), (3, "=")]),                # an insertion right after the N at 4
             (19, 24, D[19] + D[21:24], [(1, "="), (1, "D"), (3, "=")]),                  # the N at 20 is deleted
             (40, 44, "CCCC", [(4, "X")])]
    recs = ec.records(D, units)
    assert recs[0] == (1, D[0:2], "TT" + D[0], ".")
    assert recs[1] == (6, D[5], D[5] + "GGG", ".") and recs[2] == (20, D[19:21], D[19], ".")
    P = ec.apply(recs, D)
    assert [c[:2] for c in gc.clusters(recs, k)] == [(0, 2), (2, 3), (3, 4)]
    for _ in range(30):
        check_against_brute_force(D, recs, k, random_set(rng, D, P, k))
    # all of P in R: every cluster is accepted; all of D and nothing else: every cluster that adds a k-mer is rejected
    res = gc.guard(D, recs, k, qc.read_set([P.encode()], k))
    assert res.filters == ["PASS"] * 4 and res.text == P
    res = gc.guard(D, recs, k, qc.read_set([D.encode()], k))
    assert gc.missing(res.text, k, qc.read_set([D.encode()], k)) == 0 and "kmer" in res.filters


def test_whole_contig_deletion_is_not_guarded():
    D = "ACGTACGTAC"
    recs = [(1, "A", "<DEL>", "SVTYPE=DEL;END=10")]
    res = gc.guard(D, recs, 4, qc.read_set([D.encode()], 4))
    assert res.filters == ["PASS"] and res.text == "" and (res.n_clusters, res.n_records) == (0, 0)
    assert gc.info_line(4, [res]) == "[Hypo::Hypo] Info: k-mer guard (k = 4): 0 clusters of 0 records, 0 clusters (0 records) rejected"
