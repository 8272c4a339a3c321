"""CPU checker of `hypo --kmer-fix` and hypo_gpu_kset_query_fixes (DESIGN.md "k-mer fix"): the contract in plain numpy on top of
qv_checker and qv_track_checker.  It shares no code with the host library or the kernels.

S is a contig's text before the fix.  k, R, the byte rules and the windows are those of qv_checker, the intervals (start, end, n)
those of qv_track_checker.  Interval j of S is a SITE when
  (a) k <= end - start <= 2k - 1 and n == end - start - k + 1 (every window inside is missing),
  (b) the gap to the interval before and to the one after is at least k - 1 bases,
  (c) lo = start - k + 1 >= 0 and hi = end + k - 1 <= |S| (a span clipped by a contig end is never a site),
  (d) S[lo:hi) is all ACGTacgt,
  (e) c1 - c0 <= 31,
with the REGION C = [c0, c1) = [end - k, start + k), the positions every missing window of the interval contains.

A site (for the entry point: any span [lo, hi) with any region [c0, c1) inside it) has 9 w - 3 CANDIDATES, w = c1 - c0, in this
order: ("none",); ("sub", p, b), p ascending over C, b in ACGT order; ("del", p), p ascending over C; ("ins", p, b), b put in
front of p, p ascending over (c0, c1), b in ACGT order.  A candidate's text is S[lo:hi) with that one edit, and its (total,
missing) are qv_checker.seq_stats of that text.  With bases compared case-blind a candidate is CANONICAL when it is sub(p, b) and
upper(S[p]) != b, or del(p) and (p == c0 or upper(S[p - 1]) != upper(S[p])), or ins(p, b) and (p == c0 + 1 or upper(S[p - 1]) != b).
best = the canonical candidate with the fewest missing windows, the first in order among equals; zeros = the canonical candidates
with missing == 0.  A site is FIXED with best iff best's missing == 0 and zeros == 1; zeros >= 2 is AMBIGUOUS.

  candidates(c0, c1)                 the candidates in order
  cand_text(S, lo, hi, cand)         the candidate's text
  is_canonical(S, c0, cand)
  many_stats(texts, k, R)            (total[], missing[]) of many texts at once (seq_stats of each)
  query(S, lo, hi, c0, c1, k, R)     what the entry point answers: dict of none_total, none_missing, best_cand, best_total,
                                     best_missing, zeros (per site), cand_total, cand_missing (all candidates, sites back to back)
                                     and first (where every site's candidates begin, n + 1 entries)
  sites(S, k, R)                     ([(start, end, n, lo, hi, c0, c1)] of the sites, the number of intervals)
  fix(S, k, R)                       (fixes [(pos, kind, ref, alt, n)] ascending, Stats) of one contig
  apply(S, fixes)                    S with the fixes applied (positions are those of S)
  run(contigs, k, R)                 ([(name, fixed text)], the TSV's text, Stats) for [(name, S)] in draft order
  parse_tsv(text)                    [(contig, pos, kind, ref, alt, n)]
  info_line(path, k, stats)          the line stdout gains
"""
import numpy as np

import qv_checker as qc
import qv_track_checker as tc

HEADER = "#contig\tpos\tkind\tref\talt\tmissing_kmers"
MAX_REGION = 31
MAX_SPAN = 2048
_BASES = b"ACGT"


def _b(s):
    return s.encode() if isinstance(s, str) else bytes(s)


def candidates(c0, c1):
    out = [("none",)]
    out += [("sub", p, _BASES[i:i + 1]) for p in range(c0, c1) for i in range(4)]
    out += [("del", p) for p in range(c0, c1)]
    out += [("ins", p, _BASES[i:i + 1]) for p in range(c0 + 1, c1) for i in range(4)]
    assert len(out) == 9 * (c1 - c0) - 3
    return out


def cand_text(S, lo, hi, cand):
    if cand[0] == "none":
        return S[lo:hi]
    p = cand[1]
    if cand[0] == "sub":
        return S[lo:p] + cand[2] + S[p + 1:hi]
    if cand[0] == "del":
        return S[lo:p] + S[p + 1:hi]
    return S[lo:p] + cand[2] + S[p:hi]


def is_canonical(S, c0, cand):
    if cand[0] == "none":
        return False
    p = cand[1]
    up = lambda i: S[i:i + 1].upper()
    if cand[0] == "sub":
        return up(p) != cand[2]
    if cand[0] == "del":
        return p == c0 or up(p - 1) != up(p)
    return p == c0 + 1 or up(p - 1) != cand[2]


def _windows(texts, k):
    """(the text every bases-only window of the texts lies in, its canonical code), in one pass over the texts joined by a byte that
    is no base"""
    blob = b"\n".join(texts)
    first = np.concatenate([[0], np.cumsum([len(t) + 1 for t in texts])])[:len(texts)]      # where every text starts in the blob
    codes = qc._LUT[np.frombuffer(blob, dtype=np.uint8)]
    m = codes.size - k + 1
    if m <= 0:
        return np.zeros(0, np.int64), np.zeros(0, np.uint64)
    bad = np.concatenate([[0], np.cumsum(codes > 3)])
    starts = np.flatnonzero((bad[k:k + m] - bad[:m]) == 0)                         # the windows made of bases only, in order
    w = qc.canonical_windows(blob, k)
    assert w.size == starts.size
    return np.searchsorted(first, starts, side="right") - 1, w


def _count(who, w, n, R):
    total = np.bincount(who, minlength=n).astype(np.int64)
    if R.size == 0 or w.size == 0:
        return total, total.copy()
    at = np.minimum(np.searchsorted(R, w), R.size - 1)
    return total, np.bincount(who[R[at] != w], minlength=n).astype(np.int64)


def many_stats(texts, k, R):
    """seq_stats of every text, all at once"""
    if not texts:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    who, w = _windows(texts, k)
    return _count(who, w, len(texts), R)


def query(S, lo, hi, c0, c1, k, R):
    """R: one set, or a list of sets (the windows are found once): then a list of answers"""
    S = _b(S)
    texts, canon, first = [], [], [0]
    for a, b, x, y in zip(lo, hi, c0, c1):
        a, b, x, y = int(a), int(b), int(x), int(y)
        assert 0 <= a <= x < y <= b <= len(S) and y - x <= MAX_REGION and b - a <= MAX_SPAN
        cs = candidates(x, y)
        texts += [cand_text(S, a, b, c) for c in cs]
        canon += [is_canonical(S, x, c) for c in cs]
        first.append(len(texts))
    who, w = _windows(texts, k) if texts else (np.zeros(0, np.int64), np.zeros(0, np.uint64))
    outs = []
    for r in (R if isinstance(R, (list, tuple)) else [R]):
        total, missing = (x.tolist() for x in _count(who, w, len(texts), r))
        out = {key: [] for key in ("none_total", "none_missing", "best_cand", "best_total", "best_missing", "zeros")}
        for s in range(len(first) - 1):
            i0, i1 = first[s], first[s + 1]
            ok = [j for j in range(i1 - i0) if canon[i0 + j]]
            best = min(ok, key=lambda j: (missing[i0 + j], j))
            out["none_total"].append(total[i0]); out["none_missing"].append(missing[i0])
            out["best_cand"].append(best); out["best_total"].append(total[i0 + best]); out["best_missing"].append(missing[i0 + best])
            out["zeros"].append(sum(1 for j in ok if missing[i0 + j] == 0))
        out["cand_total"], out["cand_missing"], out["first"] = total, missing, first
        outs.append(out)
    return outs if isinstance(R, (list, tuple)) else outs[0]


def sites(S, k, R):
    S = _b(S)
    ivs = tc.intervals(S, k, R)
    codes = qc._LUT[np.frombuffer(S, dtype=np.uint8)]
    out = []
    for j, (start, end, n) in enumerate(ivs):
        if not (k <= end - start <= 2 * k - 1 and n == end - start - k + 1):
            continue
        if j and start - ivs[j - 1][1] < k - 1:
            continue
        if j + 1 < len(ivs) and ivs[j + 1][0] - end < k - 1:
            continue
        lo, hi = start - k + 1, end + k - 1
        if lo < 0 or hi > len(S):
            continue
        if np.any(codes[lo:hi] > 3):
            continue
        c0, c1 = end - k, start + k
        if c1 - c0 > MAX_REGION:
            continue
        out.append((start, end, n, lo, hi, c0, c1))
    return out, len(ivs)


class Stats:
    def __init__(self):
        self.intervals = self.sites = self.fixed = self.sub = self.dele = self.ins = self.ambiguous = self.removed = 0

    def add(self, o):
        for key in vars(self):
            setattr(self, key, getattr(self, key) + getattr(o, key))

    def tuple(self):
        return (self.intervals, self.sites, self.fixed, self.sub, self.dele, self.ins, self.ambiguous, self.removed)


def fix(S, k, R):
    S = _b(S)
    st = Stats()
    ss, st.intervals = sites(S, k, R)
    st.sites = len(ss)
    fixes = []
    if not ss:
        return fixes, st
    q = query(S, [s[3] for s in ss], [s[4] for s in ss], [s[5] for s in ss], [s[6] for s in ss], k, R)
    for i, (start, end, n, lo, hi, c0, c1) in enumerate(ss):
        assert q["none_missing"][i] == n and q["none_total"][i] == hi - lo - k + 1
        if q["zeros"][i] >= 2:
            st.ambiguous += 1
        if not (q["best_missing"][i] == 0 and q["zeros"][i] == 1):
            continue
        c = candidates(c0, c1)[q["best_cand"][i]]
        p = c[1]
        if c[0] == "sub":
            fixes.append((p, "sub", S[p:p + 1].decode(), c[2].decode(), n)); st.sub += 1
        elif c[0] == "del":
            fixes.append((p, "del", S[p:p + 1].decode(), ".", n)); st.dele += 1
        else:
            fixes.append((p, "ins", ".", c[2].decode(), n)); st.ins += 1
        st.fixed += 1
        st.removed += n
    assert fixes == sorted(fixes)
    return fixes, st


def apply(S, fixes):
    """positions are those of S: the fixes go in from the last to the first"""
    S = bytearray(_b(S))
    for pos, kind, ref, alt, _ in sorted(fixes, reverse=True):
        if kind == "sub":
            assert S[pos:pos + 1] == ref.encode()
            S[pos:pos + 1] = alt.encode()
        elif kind == "del":
            assert S[pos:pos + 1] == ref.encode() and alt == "."
            del S[pos]
        else:
            assert kind == "ins" and ref == "."
            S[pos:pos] = alt.encode()
    return bytes(S)


def run(contigs, k, R):
    lines, out, st = [HEADER], [], Stats()
    for name, S in contigs:
        fixes, s = fix(S, k, R)
        st.add(s)
        out.append((name, apply(S, fixes).decode()))
        lines += [f"{name}\t{pos}\t{kind}\t{ref}\t{alt}\t{n}" for pos, kind, ref, alt, n in fixes]
    return out, "\n".join(lines) + "\n", st


def parse_tsv(text):
    lines = text.split("\n")
    assert lines[0] == HEADER and lines[-1] == ""
    out = []
    for l in lines[1:-1]:
        f = l.split("\t")
        assert len(f) == 6 and f[2] in ("sub", "del", "ins"), l
        out.append((f[0], int(f[1]), f[2], f[3], f[4], int(f[5])))
    return out


def info_line(path, k, st):
    return (f"[Hypo::Hypo] Info: k-mer fix {path} (k = {k}): {st.intervals} intervals, {st.sites} sites, {st.fixed} fixed ({st.sub} sub, {st.dele} del, "
            f"{st.ins} ins), {st.ambiguous} ambiguous, {st.removed} missing k-mers removed")
