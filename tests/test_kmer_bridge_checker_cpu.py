"""CPU: tests/kmer_bridge_checker.py against brute force.  For k = 12, small sets with branches, dead ends and cycles, and dhi <= 6:
every string over ACGT of every allowed length is enumerated, those whose k-mers are all in the set and that end in R at their first
allowed arrival are the walks; their number (0, 1, 2 or more) and the first of them in A < C < G < T order are the checker's, and the
checker's steps are those of a literal transcription of the search in include/hypo_gpu.h.  Then the trim rule, and on planted cases
the text the bridges give and the identity missing(after) = missing(before) - sum of the bridged intervals' counts."""
import itertools

import numpy as np
import pytest

import kmer_bridge_checker as kb
import qv_checker as qc

K = 12
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def canon(s):
    rc = "".join(COMP[c] for c in reversed(s))
    return min(s, rc)


class Stop(Exception):
    pass


def literal(L, Rk, dlo, dhi, budget, kmers):
    """the pseudocode, word for word, on strings; kmers: the set as canonical strings"""
    state = {"steps": 0, "found": 0, "first": None, "status": None}

    def visit(x, depth, path):
        state["steps"] += 1
        if state["steps"] > budget:
            state["status"] = kb.OVER_BUDGET
            raise Stop
        if depth >= dlo and x == Rk:
            state["found"] += 1
            if state["found"] == 2:
                state["status"] = kb.AMBIGUOUS
                raise Stop
            state["first"] = path
            return
        if depth == dhi:
            return
        for b in "ACGT":
            y = x[1:] + b
            if canon(y) in kmers:
                visit(y, depth + 1, path + b)

    try:
        visit(L, 0, "")
        state["status"] = kb.UNIQUE if state["found"] == 1 else kb.NONE
    except Stop:
        pass
    return state["status"], state["steps"], state["first"]


def brute(L, Rk, dlo, dhi, kmers):
    """every walk, in A < C < G < T order"""
    out = []
    for n in range(dlo, dhi + 1):
        for w in itertools.product("ACGT", repeat=n):
            t = L + "".join(w)
            if t[n:n + K] != Rk:
                continue
            if any(t[j:j + K] == Rk for j in range(dlo, n)):
                continue
            if all(canon(t[i:i + K]) in kmers for i in range(1, n + 1)):
                out.append("".join(w))
    return sorted(out)


def make_case(rng):
    """a set from a few variants of one low-complexity string, with dead ends, and a query between two of its positions"""
    alphabet = "ACGT"[:int(rng.integers(2, 5))]
    n = 50
    tandem = rng.random() < 0.5
    if tandem:                                                             # a tandem repeat in the middle: cycles
        unit = "".join(rng.choice(list(alphabet), int(rng.integers(1, 4))))
        truth = "".join(rng.choice(list(alphabet), 15)) + (unit * 20)[:20] + "".join(rng.choice(list(alphabet), 15))
    else:
        truth = "".join(rng.choice(list(alphabet), n))
    variants = [truth]
    for _ in range(int(rng.integers(0, 4))):
        v = list(truth)
        p = int(rng.integers(14, 30))
        kind = rng.integers(0, 3)
        if kind == 0:
            v[p] = str(rng.choice(list("ACGT")))
        elif kind == 1:
            del v[p:p + int(rng.integers(1, 3))]
        else:
            v[p:p] = list(rng.choice(list("ACGT"), int(rng.integers(1, 3))))
        variants.append("".join(v))
    kmers = {canon(v[i:i + K]) for v in variants for i in range(len(v) - K + 1)}
    for km in list(kmers)[::5]:                                            # dead ends: a k-mer with another last base
        kmers.add(canon(km[:-1] + str(rng.choice(list("ACGT")))))
    src, dst = variants[int(rng.integers(len(variants)))], variants[int(rng.integers(len(variants)))]
    a = int(rng.integers(8, 24))
    d = int(rng.integers(0, 7))
    dhi = int(rng.integers(1, 7))
    dlo = int(rng.integers(1, dhi + 1))
    if tandem and rng.random() < 0.6:                                      # L inside the repeat, R over its end: once more round, or out
        src = dst = truth
        a, d, dhi = int(rng.integers(21, 24)), int(rng.integers(1, 5)), 6
        dlo = int(rng.integers(1, 3))
    L, Rk = src[a:a + K], dst[a + d:a + d + K]
    return L, Rk, dlo, dhi, kmers


def codes_of(kmers):
    return np.array(sorted({int(qc.canonical_windows(km.encode(), K)[0]) for km in kmers}), np.uint64)


def test_search_equals_brute_force_and_the_literal_search():
    rng = np.random.default_rng(20261020)
    seen = {kb.NONE: 0, kb.UNIQUE: 0, kb.AMBIGUOUS: 0, kb.OVER_BUDGET: 0}
    for trial in range(160):
        L, Rk, dlo, dhi, kmers = make_case(rng)
        R = codes_of(kmers)
        walks = brute(L, Rk, dlo, dhi, kmers)
        st, steps, walk = kb.search(L, Rk, dlo, dhi, kb.MAX_BUDGET, K, R)
        want = kb.NONE if not walks else kb.UNIQUE if len(walks) == 1 else kb.AMBIGUOUS
        assert st == want, (trial, L, Rk, dlo, dhi, walks, st)
        assert walk.decode() == (walks[0] if walks else ""), (trial, walks, walk)
        lst, lsteps, lfirst = literal(L, Rk, dlo, dhi, kb.MAX_BUDGET, kmers)
        assert (lst, lsteps, lfirst or "") == (st, steps, walk.decode()), trial
        seen[st] += 1
        # a budget of exactly the steps changes nothing; one less ends the search there
        assert kb.search(L, Rk, dlo, dhi, steps, K, R) == (st, steps, walk)
        if steps > 1:
            assert kb.search(L, Rk, dlo, dhi, steps - 1, K, R) == (kb.OVER_BUDGET, steps, b"") == literal(L, Rk, dlo, dhi, steps - 1, kmers)[:2] + (b"",)
            seen[kb.OVER_BUDGET] += 1
    assert min(seen.values()) >= 10, seen


def test_search_edges():
    truth = "ACGTTGCATGCCAGTACGGATCAAGT"
    kmers = {canon(truth[i:i + K]) for i in range(len(truth) - K + 1)}
    R = codes_of(kmers)
    L, Rk = truth[:K], truth[5:5 + K]
    assert kb.search(L, Rk, 1, 5, 100, K, R) == (kb.UNIQUE, 6, truth[K:K + 5].encode())
    assert kb.search(L.lower(), Rk.lower(), 5, 5, 100, K, R) == (kb.UNIQUE, 6, truth[K:K + 5].encode())       # case is ignored
    assert kb.search(L, Rk, 1, 4, 100, K, R) == (kb.NONE, 5, b"")                                            # one beyond dhi
    assert kb.search(L, Rk, 6, 9, 100, K, R)[0] == kb.NONE                                                   # arrives in front of dlo, walks on, never again
    assert kb.search(L[:-1] + "N", Rk, 1, 5, 100, K, R) == (kb.NOANCHOR, 0, b"") == kb.search(L, "N" + Rk[1:], 1, 5, 100, K, R)
    assert kb.search("T" + L[1:], Rk, 1, 5, 100, K, R)[0] == kb.UNIQUE                                       # L itself need not be in the set
    assert kb.search(L, Rk[:-1] + ("A" if Rk[-1] != "A" else "C"), 1, 5, 100, K, R)[0] == kb.NONE            # R must be
    # a homopolymer: L == R, the walk comes back after every single step and ends at its first allowed arrival
    hp = {canon("A" * K)}
    assert kb.search("A" * K, "A" * K, 1, 6, 100, K, codes_of(hp)) == (kb.UNIQUE, 2, b"A")
    assert kb.search("A" * K, "A" * K, 3, 6, 100, K, codes_of(hp)) == (kb.UNIQUE, 4, b"AAA")
    q = kb.query(truth, [0, 0], [5, 5], [1, 1], [5, 4], 100, K, R)
    assert q == {"status": [kb.UNIQUE, kb.NONE], "steps": [6, 5], "len": [5, 0], "walk": [truth[K:K + 5].encode(), b""]}


def test_trim_rule():
    assert kb.trim(b"AAACGTTT", b"AAAGTTT") == (3, b"C", b"")
    assert kb.trim(b"aaacgttt", b"AAAGGTTT") == (3, b"c", b"G")                   # case-blind; ref keeps its case
    assert kb.trim(b"ACAAAAAT", b"ACAAAAAAAT") == (7, b"", b"AA")                 # the prefix first: a run's new bases go to its end
    assert kb.trim(b"ACAAAAAT", b"ACAAAT") == (5, b"AA", b"")
    assert kb.trim(b"ACGTACGT", b"ACCTAGGT") == (2, b"GTAC", b"CTAG")             # two substitutions: one edit from the first to the last
    assert kb.trim(b"ACGT", b"ACGT") == (4, b"", b"")


@pytest.mark.parametrize("M,D", [(64, 8), (40, 3)])
def test_planted_cases(M, D):
    rng = np.random.default_rng(7)
    truth = "".join(rng.choice(list("ACGT"), 400))
    truth = truth[:300] + "CAAAAAAAG" + truth[309:]                       # a homopolymer run at 301..307
    R = qc.read_set([truth.encode()], K)
    s = list(truth)
    s[300:309] = list("CAAAAAG")                                           # the run two bases short
    s[240:243] = [next(c for c in "ACGT" if c not in truth[240:242]), truth[242]]     # a substitution and a deletion next to it
    s[180:184] = [("G" if truth[180] != "G" else "T"), truth[181], truth[182], ("G" if truth[183] != "G" else "T")]   # two substitutions 3 apart
    s[120:120] = list("GAT")                                               # 3 bases too many
    del s[60:62]                                                           # 2 bases missing
    S = "".join(s)
    edits, st = kb.bridge(S, K, R, M, D)
    assert st.sites == st.intervals == 5 and st.bridged == 5 and st.ambiguous == 0 and st.over_budget == 0, st.tuple()
    assert kb.apply(S, edits).decode() == truth
    tb, mb = qc.seq_stats(S, K, R)
    ta, ma = qc.seq_stats(kb.apply(S, edits), K, R)
    assert ma == 0 and mb - ma == st.removed == sum(e[3] for e in edits)
    alt_len = lambda e: 0 if e[2] == "." else len(e[2])
    ref_len = lambda e: 0 if e[1] == "." else len(e[1])
    assert ta - tb == sum(alt_len(e) - ref_len(e) for e in edits) == st.bases_in - st.bases_out
    assert sorted((ref_len(e), alt_len(e)) for e in edits) == sorted([(0, 2), (3, 0), (4, 4), (1, 2), (0, 2)])
    # a length change beyond the slack is left alone, and so is an anchor distance beyond M
    e0, st0 = kb.bridge(S, K, R, M, 1)
    assert st0.bridged == 2 and [ref_len(e) for e in e0] == [4, 1]
    e1, st1 = kb.bridge(S, K, R, 12, D)
    assert st1.intervals == 5 and st1.sites < 5
    contigs = [("one", S), ("two", truth), ("three", S.lower())]
    out, tsv, sts = kb.run(contigs, K, R, M, D)
    assert [o[1].upper() for o in out] == [truth] * 3 and sts.bridged == 10 and out[2][1] != truth
    rows = kb.parse_tsv(tsv)
    assert [r[0] for r in rows] == ["one"] * 5 + ["three"] * 5 and [r[1:] for r in rows[:5]] == edits
    assert kb.info_line("b.tsv", K, M, D, sts) == (f"[Hypo::Hypo] Info: k-mer bridge b.tsv (k = 12, max {M}, slack {D}): 10 intervals, 10 sites, 10 bridged "
                                                  f"({sts.bases_out} bases out, {sts.bases_in} bases in), 0 ambiguous, 0 over budget, {sts.removed} missing k-mers removed")
