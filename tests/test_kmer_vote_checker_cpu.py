"""CPU: tests/kmer_vote_checker.py against brute force.  The cases are those of tests/test_kmer_bridge_checker_cpu.py (k = 12, small
sets with branches, dead ends and cycles, dhi <= 6), every k-mer with a count of its own: every string over ACGT of every allowed
length is enumerated, those whose k-mers all count at least t and that end in R at their first allowed arrival are the walks, in
A < C < G < T order, each with the least count among its k-mers at depths 1 .. len; search_set reports the first four of them, NONE /
UNIQUE / AMBIGUOUS / MANY by their number, and its steps are those of a literal transcription of the search in include/hypo_gpu.h.
Where neither search hits the budget, its first walk and its NONE / UNIQUE verdict are kmer_bridge_checker.search's.  Then decide at
its edges, and the vote over a planted text."""
import numpy as np
import pytest

import kmer_bridge_checker as kb
import kmer_vote_checker as kv
from test_kmer_bridge_checker_cpu import K, Stop, brute, canon, make_case


def code(s):
    return min(kb._codes(s.encode()))


def literal(L, Rk, dlo, dhi, budget, counts, t):
    """the pseudocode, word for word, on strings; counts: {canonical string: count}"""
    state = {"steps": 0, "walks": [], "status": None}

    def visit(x, depth, path, lo):
        state["steps"] += 1
        if state["steps"] > budget:
            state["status"] = kb.OVER_BUDGET
            raise Stop
        if depth >= dlo and x == Rk:
            if len(state["walks"]) == kv.W:
                state["status"] = kv.MANY
                raise Stop
            state["walks"].append((path.encode(), lo))
            return
        if depth == dhi:
            return
        for b in "ACGT":
            y = x[1:] + b
            c = counts.get(canon(y), 0)
            if c >= t:
                visit(y, depth + 1, path + b, min(lo, c))

    try:
        visit(L, 0, "", 255)
        state["status"] = (kb.NONE, kb.UNIQUE, kb.AMBIGUOUS)[min(len(state["walks"]), 2)]
    except Stop:
        pass
    if state["status"] == kb.OVER_BUDGET:
        state["walks"] = []
    return state["status"], state["steps"], state["walks"]


def counted_case(rng):
    L, Rk, dlo, dhi, kmers = make_case(rng)
    counts = {km: int(rng.choice([1, 1, 2, 3, 7, 40, 255])) for km in sorted(kmers)}
    return L, Rk, dlo, dhi, counts


@pytest.mark.parametrize("seed", range(6))
def test_search_set_is_brute_force_and_the_pseudocode(seed):
    rng = np.random.default_rng(700 + seed)
    seen = set()
    for _ in range(60):
        L, Rk, dlo, dhi, counts = counted_case(rng)
        C = {code(km): c for km, c in counts.items()}
        for t in (1, 2, 3):
            kmers = {km for km, c in counts.items() if c >= t}
            walks = brute(L, Rk, dlo, dhi, kmers)
            low = lambda w: min(counts[canon((L + w)[i:i + K])] for i in range(1, len(w) + 1))
            want = [(w.encode(), low(w)) for w in walks]
            st, steps, got = kv.search_set(L, Rk, dlo, dhi, kb.MAX_BUDGET, K, C, t)
            assert got == want[:kv.W], (L, Rk, dlo, dhi, t)
            assert st == (kv.MANY if len(want) > kv.W else (kb.NONE, kb.UNIQUE, kb.AMBIGUOUS)[min(len(want), 2)])
            assert (st, steps, got) == literal(L, Rk, dlo, dhi, kb.MAX_BUDGET, counts, t)
            seen.add(st)
            # the budget: exactly the steps changes nothing, one less is BUDGET with no walk
            assert kv.search_set(L, Rk, dlo, dhi, steps, K, C, t) == (st, steps, got)
            if steps > 1:
                assert kv.search_set(L, Rk, dlo, dhi, steps - 1, K, C, t) == (kb.OVER_BUDGET, steps, []) == literal(L, Rk, dlo, dhi, steps - 1, counts, t)
            # the walks entry's search on R_t: the same first walk and the same NONE / UNIQUE verdict
            st1, steps1, first = kb.search(L, Rk, dlo, dhi, kb.MAX_BUDGET, K, {code(km) for km in kmers})
            assert first == (got[0][0] if got else b"")
            assert (st1 == kb.NONE) == (st == kb.NONE) and (st1 == kb.UNIQUE) == (st == kb.UNIQUE)
            if st1 in (kb.NONE, kb.UNIQUE):
                assert steps1 == steps
    assert {kb.NONE, kb.UNIQUE, kb.AMBIGUOUS} <= seen


def test_many_and_noanchor():
    """a set that holds every k-mer over {A, C}, from poly-A back to poly-A: the walks are A, and every string that starts and ends with
    C and holds no run of K As, followed by K As; and anchors that hold no base"""
    import itertools
    C = {code("".join(w)): 9 for w in itertools.product("AC", repeat=K)}
    C[code("A" * K)] = 200
    L = Rk = "A" * K
    A = b"A" * K
    assert kv.search_set(L, Rk, 1, 1, 100, K, C) == (kb.UNIQUE, 3, [(b"A", 200)])           # the visits of L, A and C
    st, steps, walks = kv.search_set(L, Rk, 1, K + 2, kb.MAX_BUDGET, K, C)
    assert (st, walks) == (kb.AMBIGUOUS, [(b"A", 200), (b"C" + A, 9), (b"CC" + A, 9)])
    st, steps, walks = kv.search_set(L, Rk, 1, K + 3, kb.MAX_BUDGET, K, C)
    assert (st, walks) == (kv.MANY, [(b"A", 200), (b"C" + A, 9), (b"CAC" + A, 9), (b"CC" + A, 9)])      # CCC + A is the fifth
    assert kv.search_set(L, Rk, 1, K + 3, kb.MAX_BUDGET, K, C, 10) == (kb.UNIQUE, 2, [(b"A", 200)])     # under t = 10 only poly-A counts
    assert kv.search_set(L, Rk[:-1] + "N", 1, 4, 100, K, C) == (kb.NOANCHOR, 0, [])
    assert kv.search_set("n" + L[1:], Rk, 1, 4, 100, K, C) == (kb.NOANCHOR, 0, [])
    assert kv.search_set(L.lower(), Rk, 1, 1, 100, K, C)[2] == [(b"A", 200)]


def test_decide():
    w = lambda *lows: [(bytes([65 + i]), c) for i, c in enumerate(lows)]
    assert kv.decide(w(30, 1), 4) == (0, 30, 1)
    assert kv.decide(w(1, 30), 4) == (1, 30, 1)
    assert kv.decide(w(8, 2), 4) == (0, 8, 2)                              # c1 = ratio * c2
    assert kv.decide(w(7, 2), 4) == (None, 7, 2)                           # one below
    assert kv.decide(w(2, 7), 4) == (None, 7, 2)
    assert kv.decide(w(5, 5), 2) == (None, 5, 5)                           # ties
    assert kv.decide(w(1, 1), 2) == (None, 1, 1)
    assert kv.decide(w(255, 255), 2) == (None, 255, 255)                   # saturated: both stop at 255, however far apart they were
    assert kv.decide(w(255, 127), 2) == (0, 255, 127)
    assert kv.decide(w(255, 128), 2) == (None, 255, 128)
    assert kv.decide(w(255, 1), 255) == (0, 255, 1)
    assert kv.decide(w(254, 1), 255) == (None, 254, 1)
    assert kv.decide(w(1, 2, 50, 3), 4) == (2, 50, 3)                      # W walks: the best against the second best
    assert kv.decide(w(1, 50, 50, 3), 4) == (None, 50, 50)
    assert kv.decide(w(20, 2, 1, 80), 4) == (3, 80, 20)
    assert kv.decide(w(21, 2, 1, 80), 4) == (None, 80, 21)
    for bad in (w(3), w(1, 2, 3, 4, 5)):
        with pytest.raises(AssertionError):
            kv.decide(bad, 4)
    for ratio in (1, 256):
        with pytest.raises(AssertionError):
            kv.decide(w(9, 1), ratio)


def test_vote_over_a_planted_text():
    """a truth read about 30 times, two pairs of planted substitutions 6 apart with reads that carry another base between them, once
    (an error) and 20 times (an allele), and one planted substitution on its own: the bridge alone leaves the pairs ambiguous, the vote
    chooses the truth where the other walk is an error, not where both are well supported"""
    import qv_checker as qc
    k = 15
    rng = np.random.default_rng(5)
    truth = "".join(rng.choice(list("ACGT"), 1200))
    other = lambda c: "ACGT"[("ACGT".index(c) + 1) % 4]
    sub = lambda s, p: s[:p] + other(s[p]) + s[p + 1:]
    reads = [truth[i:i + 100] for i in range(0, 1101)][::3]                # a k-mer is in 28 or 29 of them
    reads += [sub(truth, 303)[260:360]]                                    # an error between the planted edits at 300 and 306
    reads += [sub(truth, 603)[560:660]] * 20                               # a second allele between the planted edits at 600 and 606
    text = truth
    for p in (300, 306, 600, 606, 900):                                    # the one at 900 has one walk
        text = sub(text, p)
    C = kv.read_count_map([r.encode() for r in reads], k)
    R = np.array(sorted(C), np.uint64)
    edits0, st0 = kb.bridge(text, k, R)
    assert (st0.sites, st0.bridged, st0.ambiguous) == (3, 1, 2)
    edits, st, vt = kv.bridge_vote(text, k, C, 1, 4)
    assert vt.tuple() == (2, 1, 1, 0, 0) and (st.sites, st.bridged, st.ambiguous) == (3, 2, 1)
    assert [e[:4] for e in edits if e[5] == 1] == [e[:4] for e in edits0]
    chosen = [e for e in edits if e[5] > 1]
    assert len(chosen) == 1 and chosen[0][0] == 300 and chosen[0][5] == 2 and chosen[0][6].endswith("/1")
    new = kb.apply(text, [e[:5] for e in edits]).decode()
    assert new == sub(sub(truth, 600), 606)                               # the sites at 300 and 900 are the truth again, the close one stays
    # the identity: the missing k-mers drop by the bridged and chosen sites' counts
    miss = lambda s: qc.seq_stats(s, k, R)[1]
    assert miss(new) == miss(text) - sum(e[3] for e in edits)
    # at ratio 2 the second allele's site is still too close (28 against 20), and under t = 2 the error is gone: that site is unique
    assert kv.bridge_vote(text, k, C, 1, 2)[2].tuple() == (2, 1, 1, 0, 0)
    edits2, st2, vt2 = kv.bridge_vote(text, k, C, 2, 4)
    assert vt2.tuple() == (1, 0, 1, 0, 0) and st2.bridged == 2 and [e[:4] for e in edits2] == [e[:4] for e in edits]
    # the TSV and the lines
    out, tsv, s, v = kv.run([("c1", text)], k, C, 1, 4)
    assert out == [("c1", new)] and s.tuple() == st.tuple() and v.tuple() == vt.tuple()
    rows = kv.parse_tsv(tsv)
    assert [r[1:] for r in rows] == edits and tsv.startswith("#contig\tpos\tref\talt\tmissing_kmers\tsteps\twalks\tsupport\n")
    lines = kv.info_lines("b.tsv", k, 64, 8, 4, s, v)
    assert lines[0] == kb.info_line("b.tsv", k, 64, 8, s)
    assert lines[1] == "[Hypo::Hypo] Info: k-mer bridge vote (ratio 4, up to 4 walks): 2 asked, 1 chosen, 1 too close, 0 more than 4 walks, 0 over budget"
