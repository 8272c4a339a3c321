"""CPU: tests/kmer_fix_checker.py pinned by brute force.  A random genome with homopolymer runs is the reads' set; the text is the
genome with single errors planted far apart.  Every candidate's string is built here, with Python's own slicing, and asked with
qv_checker.seq_stats one at a time; the checker's vectorised pairs, its canonical rule, its sites and its decisions must agree, and
the missing k-mers of the fixed text drop by exactly the fixed intervals' counts."""
import numpy as np
import pytest

import kmer_fix_checker as fc
import qv_checker as qc
import qv_track_checker as tc

KS = [12, 21]


def rnd(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n))


def genome_of(rng, n):
    g = bytearray(rnd(rng, n))
    for at in range(97, n - 20, 211):                                    # homopolymer runs of 3 to 8
        g[at:at + 3 + at % 6] = bytes([g[at]]) * (3 + at % 6)
    return bytes(g)


def plant(rng, genome, k, step):
    """(text, [(kind, position in the text)]): one error every `step` bases, kinds in turn, every fourth inside a homopolymer run"""
    out, planted, at, i = bytearray(), [], 0, 0
    for p in range(4 * k, len(genome) - 4 * k, step):
        if i % 4 == 3:                                                   # move into the next run of at least 3 equal bases
            q = next((q for q in range(p, p + step // 2) if genome[q] == genome[q + 1] == genome[q + 2]), p)
            p = q + 1
        out += genome[at:p]
        kind = ("sub", "del", "ins")[i % 3]
        planted.append((kind, len(out)))
        if kind == "sub":
            out += bytes([b"ACGT"[(b"ACGT".index(genome[p]) + 1 + i % 3) % 4]]); at = p + 1
        elif kind == "del":
            at = p + 1
        else:
            out += bytes([b"ACGT"[i % 4]]); at = p
        i += 1
    out += genome[at:]
    return bytes(out), planted


_cases = {}


def case(k):
    if k not in _cases:
        rng = np.random.default_rng(700 + k)
        genome = genome_of(rng, 9000)
        text, planted = plant(rng, genome, k, 4 * k + 37)
        _cases[k] = (genome, qc.read_set([genome], k), text, planted)
    return _cases[k]


def brute(S, lo, hi, c0, c1, k, R):
    """per candidate (string, (total, missing)), strings built by hand"""
    out = [(S[lo:hi], qc.seq_stats(S[lo:hi], k, R))]
    for p in range(c0, c1):
        for b in b"ACGT":
            s = S[lo:p] + bytes([b]) + S[p + 1:hi]
            out.append((s, qc.seq_stats(s, k, R)))
    for p in range(c0, c1):
        s = S[lo:p] + S[p + 1:hi]
        out.append((s, qc.seq_stats(s, k, R)))
    for p in range(c0 + 1, c1):
        for b in b"ACGT":
            s = S[lo:p] + bytes([b]) + S[p:hi]
            out.append((s, qc.seq_stats(s, k, R)))
    return out


@pytest.mark.parametrize("k", KS)
def test_candidates_pairs_and_canonical(k):
    genome, R, S, planted = case(k)
    ss, n_iv = fc.sites(S, k, R)
    assert len(ss) >= 20 and n_iv >= len(ss)
    q = fc.query(S, [s[3] for s in ss], [s[4] for s in ss], [s[5] for s in ss], [s[6] for s in ss], k, R)
    at = 0
    for i, (start, end, n, lo, hi, c0, c1) in enumerate(ss):
        assert (c0, c1) == (end - k, start + k) and 1 <= c1 - c0 <= k and (lo, hi) == (start - k + 1, end + k - 1)
        cands = fc.candidates(c0, c1)
        b = brute(S, lo, hi, c0, c1, k, R)
        assert len(b) == len(cands) == 9 * (c1 - c0) - 3
        assert [x[0] for x in b] == [fc.cand_text(S, lo, hi, c) for c in cands]
        assert [x[1][0] for x in b] == q["cand_total"][at:at + len(b)] and [x[1][1] for x in b] == q["cand_missing"][at:at + len(b)]
        at += len(b)
        canon = [fc.is_canonical(S, c0, c) for c in cands]
        assert not canon[0]
        texts = [x[0].upper() for x in b]
        ctexts = [t for t, c in zip(texts, canon) if c]
        assert len(set(ctexts)) == len(ctexts), "two canonical candidates spell one text"
        assert texts[0] not in ctexts
        for t, c in zip(texts[1:], canon[1:]):
            assert c or t == texts[0] or t in ctexts
        ok = [j for j, c in enumerate(canon) if c]
        best = min(ok, key=lambda j: (b[j][1][1], j))
        assert (q["best_cand"][i], q["best_total"][i], q["best_missing"][i]) == (best, b[best][1][0], b[best][1][1])
        assert q["zeros"][i] == sum(1 for j in ok if b[j][1][1] == 0)
        assert (q["none_total"][i], q["none_missing"][i]) == b[0][1] == (hi - lo - k + 1, n)
    assert at == len(q["cand_total"])


@pytest.mark.parametrize("k", KS)
def test_planted_errors_are_fixed(k):
    genome, R, S, planted = case(k)
    fixes, st = fc.fix(S, k, R)
    assert st.fixed == len(fixes) and st.fixed == st.sub + st.dele + st.ins and min(st.sub, st.dele, st.ins) >= 3
    assert st.fixed >= 0.8 * len(planted) and st.sites <= st.intervals
    fixed = fc.apply(S, fixes)
    t0, m0 = qc.seq_stats(S, k, R)
    t1, m1 = qc.seq_stats(fixed, k, R)
    assert m1 == m0 - sum(f[4] for f in fixes) == m0 - st.removed
    if st.fixed == len(planted):
        assert fixed == genome
    # the lines of the file, applied from the last to the first, are the same text
    out, tsv, st2 = fc.run([("a", S), ("b", genome), ("c", S[:300])], k, R)
    rows = fc.parse_tsv(tsv)
    assert [r[1:] for r in rows if r[0] == "a"] == fixes and not [r for r in rows if r[0] == "b"]
    assert out[0] == ("a", fixed.decode()) and out[1] == ("b", genome.decode())
    back = bytearray(S)
    for _, pos, kind, ref, alt, _ in reversed([r for r in rows if r[0] == "a"]):
        back[pos:pos + (kind != "ins")] = b"" if kind == "del" else alt.encode()
    assert bytes(back) == fixed
    assert st2.tuple()[2:] == tuple(a + b for a, b in zip(st.tuple()[2:], fc.fix(S[:300], k, R)[1].tuple()[2:]))
    line = fc.info_line("f.tsv", k, st)
    assert line.startswith("[Hypo::Hypo] Info: k-mer fix f.tsv (k = %d): %d intervals, %d sites, %d fixed (" % (k, st.intervals, st.sites, st.fixed))
    # a second pass finds nothing more to fix
    assert not fc.fix(fixed, k, R)[0]


@pytest.mark.parametrize("k", KS)
def test_what_is_no_site(k):
    rng = np.random.default_rng(900 + k)
    genome = rnd(rng, 2000)
    R = qc.read_set([genome], k)
    flip = lambda s, p: s[:p] + bytes([b"ACGT"[(b"ACGT".index(s[p]) + 1) % 4]]) + s[p + 1:]

    def site_starts(S, R=R):
        return [s[0] for s in fc.sites(S, k, R)[0]]

    def interval_at(S, p, R=R):
        return [iv for iv in tc.intervals(S, k, R) if iv[0] <= p < iv[1]]

    plain = flip(genome, 1000)
    assert site_starts(plain) == [1000 - k + 1] and interval_at(plain, 1000) == [(1000 - k + 1, 1000 + k, k)]
    # clipped by either end of the contig: the span would begin before the text or end behind it
    for p in (2 * k - 3, k - 2, 3, len(genome) - 2 * k + 2, len(genome) - k + 1, len(genome) - 2):
        S = flip(genome, p)
        assert interval_at(S, p) and site_starts(S) == []
    S = flip(genome, 2 * k - 2)                                          # the first position whose span fits: lo == 0
    assert fc.sites(S, k, R)[0][0][3] == 0
    S = flip(genome, len(genome) - 2 * k + 1)
    assert fc.sites(S, k, R)[0][0][4] == len(genome)
    # an N inside the span but outside the interval
    for d in (k + 1, -(k + 1), 2 * k - 2):
        S = bytearray(plain); S[1000 + d] = ord("N")
        assert interval_at(bytes(S), 1000) and site_starts(bytes(S)) == []
    S = bytearray(plain); S[1000 + 2 * k - 1] = ord("N")                 # just outside the span
    assert site_starts(bytes(S)) == [1000 - k + 1]
    # two intervals closer than k - 1
    for d, n_sites in ((2 * k - 1 + k - 2, 0), (2 * k - 1 + k - 1, 2)):
        S = flip(plain, 1000 + d)
        ivs = tc.intervals(S, k, R)
        assert len(ivs) == 2 and ivs[1][0] - ivs[0][1] == d - (2 * k - 1)
        assert len(site_starts(S)) == n_sites
    # a window inside the interval that is present: n < end - start - k + 1
    extra = np.unique(np.concatenate([R, qc.read_set([plain[1000 - 4:1000 - 4 + k]], k)]))
    iv = interval_at(plain, 1000, extra)
    assert iv == [(1000 - k + 1, 1000 + k, k - 1)] and site_starts(plain, extra) == []
    # longer than 2k - 1: two errors whose windows overlap
    S = flip(plain, 1003)
    assert interval_at(S, 1000)[0][1] - interval_at(S, 1000)[0][0] == 2 * k + 2 and site_starts(S) == []
