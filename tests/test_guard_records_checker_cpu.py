"""CPU: tests/guard_records_checker.py (the contract of `hypo --guard-records`) pinned by brute force on small hand-made contigs: the
checker's text has the fewest missing k-mers over ALL joint subsets of the records of the clusters it decides record by record, the
tie rules hold (most records, then the greatest mask), it is never worse than guard_checker's whole-cluster decision, and N = 1 is
that decision."""
import itertools

import numpy as np
import pytest

import edit_checker as ec
import guard_checker as gc
import guard_records_checker as grc
import qv_checker as qc

K, N = 12, 3


def rnd(seed, n):
    return "".join("ACGT"[i] for i in np.random.default_rng(seed).integers(0, 4, n))


def other(c):
    return "ACGT"[("ACGT".index(c) + 1) % 4]


def sub(D, at, good=True):
    """a substitution at draft position `at`; a bad one differs from the good one"""
    return (at + 1, D[at], other(D[at]) if good else other(other(D[at])), ".")


@pytest.fixture(scope="module")
def contig():
    """D, its records (clusters of 1, 2, 3, N + 1 = 4 and 1 records), which of them lead to the truth, and R = the truth's k-mers"""
    D = rnd(7, 300)
    recs, good = [], []

    def add(r, g=True):
        recs.append(r)
        good.append(g)
    add(sub(D, 0))                                                        # a record at position 0, alone
    add(sub(D, 50)); add(sub(D, 51, good=False), False)                   # two abutting records, the second one wrong
    add((101, D[100], D[100] + "GT", "."))                                # an insertion with its padding base,
    add(sub(D, 105, good=False), False); add((111, D[110:113], D[110], "."))   # a wrong substitution, a deletion: a cluster of 3
    add(sub(D, 180)); add(sub(D, 185)); add(sub(D, 190, good=False), False); add(sub(D, 195))   # N + 1 records: decided whole
    add((299, D[298:300], D[298], "."))                                   # a deletion that ends at the contig's end
    T = ec.apply([r for r, g in zip(recs, good) if g], D)
    R = qc.read_set([T.encode()], K)
    cl = gc.clusters(recs, K)
    assert [c[1] - c[0] for c in cl] == [1, 2, 3, 4, 1]
    assert recs[2][0] - 1 == recs[1][0] - 1 + len(recs[1][1])            # abutting
    return D, recs, good, R, cl


def test_fewest_missing_over_all_subsets(contig):
    D, recs, good, R, cl = contig
    res = grc.guard(D, recs, K, R, N)
    whole = gc.guard(D, recs, K, R)
    free = [i for c in cl if c[1] - c[0] <= N for i in range(c[0], c[1])]
    fixed = [i for c in cl if c[1] - c[0] > N for i in range(c[0], c[1]) if whole.filters[i] == "PASS"]
    assert len(free) == 7
    best = min(gc.missing(ec.apply([recs[i] for i in sorted(fixed + list(s))], D), K, R)
               for n in range(len(free) + 1) for s in itertools.combinations(free, n))
    assert gc.missing(res.text, K, R) == best
    assert res.text == ec.apply([r for r, f in zip(recs, res.filters) if f == "PASS"], D)
    # the wrong records of the small clusters go, their neighbours stay; the cluster of N + 1 records is decided whole
    assert res.filters[:6] == ["PASS", "PASS", "kmer", "PASS", "kmer", "PASS"] and res.filters[10] == "PASS"
    assert len(set(res.filters[6:10])) == 1 and res.filters[6:10] == whole.filters[6:10]
    assert res.masks == [None, 0b01, 0b101, None, None]
    assert (res.n_clusters, res.n_records, res.rej_part) == (5, 11, 2)
    assert res.rej_records == res.filters.count("kmer") and res.rej_whole == (1 if res.filters[6] == "kmer" else 0)
    assert res.sizes == {1: 2, 2: 1, 3: 1, 0: 1}
    # clusters are independent: missing(final) = missing(D) + the clusters' changes
    assert gc.missing(res.text, K, R) == gc.missing(D, K, R) + sum(a - r for r, a in res.scores)
    assert grc.info_line(K, N, [res]) == (f"[Hypo::Hypo] Info: k-mer guard (k = {K}, by record in clusters of up to {N}): 5 clusters of 11 records, "
                                          f"{res.rej_whole} clusters rejected whole, 2 in part, {res.rej_records} records rejected")


def test_never_worse_than_whole_clusters_and_n1_is_the_old_guard(contig):
    D, recs, good, R, cl = contig
    whole = gc.guard(D, recs, K, R)
    for n in (2, 3, 4, 12):
        res = grc.guard(D, recs, K, R, n)
        assert gc.missing(res.text, K, R) <= gc.missing(whole.text, K, R)
        for (r, got), (r_c, a_c) in zip(res.scores, whole.scores):
            assert r == r_c and got <= min(r_c, a_c)
    assert gc.missing(grc.guard(D, recs, K, R, 4).text, K, R) < gc.missing(whole.text, K, R)     # the wrong record of the cluster of 4 goes alone
    one = grc.guard(D, recs, K, R, 1)
    assert (one.filters, one.text, one.n_clusters, one.n_records, one.rej_whole, one.rej_records, one.rej_part) == \
           (whole.filters, whole.text, whole.n_clusters, whole.n_records, whole.rej_clusters, whole.rej_records, 0)
    assert one.masks == [None] * 5


def test_variant_texts_are_the_spans_of_the_old_guard(contig):
    D, recs, good, R, cl = contig
    P = ec.apply(recs, D)
    for c in cl:
        ref, alt = gc.spans(D, P, c, K)
        assert grc.variant_text(D, recs, c, 0, K) == ref and grc.variant_text(D, recs, c, (1 << (c[1] - c[0])) - 1, K) == alt
    c = cl[2]
    only_del = ec.apply([recs[5]], D)
    assert grc.variant_text(D, recs, c, 0b100, K) == only_del[c[2] - K + 1:c[3] - 2 + K - 1]


def test_tie_rules():
    assert grc.best([3, 1, 1, 2]) == 2                   # fewest missing, then (equal records) the greatest mask
    assert grc.best([0, 0, 0, 0]) == 3                   # then most records
    assert grc.best([1, 1, 1, 0, 1, 1, 1, 0]) == 7
    assert grc.best([0, 0, 0, 1, 0, 1, 1, 1]) == 4       # one record each: the greatest mask
    assert grc.best([5]) == 0
    D = rnd(11, 120)
    a, b = sub(D, 60), sub(D, 64)
    recs = [a, b]
    # the reads hold the draft and the polish: nothing is missing either way, a tie takes the polish (n = 1 and n = 2)
    R = qc.read_set([D.encode(), ec.apply(recs, D).encode()], K)
    res = grc.guard(D, recs, K, R, 8)
    assert res.masks == [0b11] and res.filters == ["PASS", "PASS"] and res.scores == [(0, 0)]
    R1 = qc.read_set([D.encode(), ec.apply([a], D).encode()], K)
    assert grc.guard(D, [a], K, R1, 8).filters == gc.guard(D, [a], K, R1).filters == ["PASS"] and gc.guard(D, [a], K, R1).scores == [(0, 0)]
    # the reads hold either record alone: equal missing, equal records, the later record wins
    R = qc.read_set([ec.apply([a], D).encode(), ec.apply([b], D).encode()], K)
    m, got, miss = grc.choose(D, recs, gc.clusters(recs, K)[0], K, R)
    assert miss[1] == miss[2] == 0 and miss[0] > 0 and miss[3] > 0 and m == 0b10
    assert grc.guard(D, recs, K, R, 8).filters == ["kmer", "PASS"]
    # no k-mer of the contig is in the reads: the shortest text has the fewest windows; the substitution is free and is taken
    R = qc.read_set([b"A" * 40], K)
    recs = [(61, D[60], D[60] + "TT", "."), sub(D, 64), (68, D[67:69], D[67], ".")]
    res = grc.guard(D, recs, K, R, 8)
    assert res.masks == [0b110] and res.filters == ["kmer", "PASS", "PASS"]


def test_whole_contig_deletion_is_not_guarded():
    D = rnd(13, 60)
    recs = [(1, D[0], "<DEL>", f"SVTYPE=DEL;END={len(D)}")]
    res = grc.guard(D, recs, K, qc.read_set([D.encode()], K), 8)
    assert res.filters == ["PASS"] and res.text == "" and res.n_clusters == 0 and res.masks == []


def test_site_variants():
    data, alts = b"AACCGGTTAACC", b"xyzw"
    v = grc.site_variants(data, alts, 2, 10, [(2, 4, 0, 1), (4, 4, 1, 2), (8, 10, 4, 0)])
    assert v == [b"CCGGTTAA", b"xGGTTAA", b"CCyzGGTTAA", b"xyzGGTTAA", b"CCGGTT", b"xGGTT", b"CCyzGGTT", b"xyzGGTT"]
    assert grc.site_variants(data, alts, 3, 3, []) == [b""]
