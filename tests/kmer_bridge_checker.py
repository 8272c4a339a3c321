"""CPU checker of `hypo --kmer-bridge` and hypo_gpu_kset_query_walks (DESIGN.md "k-mer bridge"): the contract in plain Python / numpy
on top of qv_checker and qv_track_checker.  It shares no code with the host library or the kernels.

k, R, the byte rules and the windows are those of qv_checker, the intervals (start, end, n) those of qv_track_checker.  R is a de
Bruijn graph: a k-mer x has the children y = x[1:] + b, b in ACGT order, whose canonical code is in R.  The WALKS of a query
(L, Rk, dlo, dhi, budget) are what this search finds, and its answer is the search's and nothing else:

    steps = found = 0
    visit(x, depth, path):
        steps += 1;  if steps > budget: stop with BUDGET
        if depth >= dlo and x == Rk:  found += 1;  if found == 2: stop with AMBIGUOUS;  first = path;  return
        if depth == dhi: return
        for b in A, C, G, T:  y = x[1:] + b;  if canonical(y) in R: visit(y, depth + 1, path + b)
    visit(L, 0, "");  status = UNIQUE if found == 1 else NONE

NOANCHOR (steps 0): an anchor holds a byte outside ACGTacgt.  len and the walk are the first arrival's for UNIQUE and AMBIGUOUS, 0
and empty otherwise; steps is budget + 1 for BUDGET.

S is a contig's text before the pass, M the largest anchor distance, D the slack.  With a = start - 1, b = end - k + 1, d0 = b - a,
interval j is a SITE when a >= 0, b + k <= |S|, 2 <= d0 <= M, S[a, a + k) and S[b, b + k) are all ACGTacgt, and at least 2 bases lie
between the interval and each neighbouring interval.  Its query: from = a, to = b, dlo = max(1, d0 - D), dhi = d0 + D, budget 4096.
It is BRIDGED iff the status is UNIQUE.  old = S[a, b + k), new = S[a, a + k) + walk; the longest case-blind common prefix goes,
then the longest case-blind common suffix of what remains; pos = a + prefix, ref / alt the remainders ("." when empty), and the text
becomes S[:pos] + alt + S[pos + |ref|:].

  as_set(R)                                   R as something `in` is quick on (search and query take it as well as the array)
  search(L, Rk, dlo, dhi, budget, k, R)       (status, steps, walk bytes) of one query; L, Rk: byte strings of k bases
  query(S, frm, to, dlo, dhi, budget, k, R)   what the entry point answers: dict of status, steps, len (lists) and walk (byte strings)
  sites(S, k, R, M)                           ([(start, end, n, a, b, d0)] of the sites, the number of intervals)
  trim(old, new)                              (prefix, ref, alt)
  bridge(S, k, R, M, D)                       (edits [(pos, ref, alt, n, steps)] ascending, Stats) of one contig
  apply(S, edits)                             S with the edits applied (positions are those of S)
  run(contigs, k, R, M, D)                    ([(name, new text)], the TSV's text, Stats) for [(name, S)] in draft order
  parse_tsv(text)                             [(contig, pos, ref, alt, n, steps)]
  info_line(path, k, M, D, stats)             the line stdout gains
"""
import numpy as np

import qv_checker as qc
import qv_track_checker as tc

HEADER = "#contig\tpos\tref\talt\tmissing_kmers\tsteps"
MAX_WALK = 256
MAX_BUDGET = 65536
BUDGET = 4096
NONE, UNIQUE, AMBIGUOUS, OVER_BUDGET, NOANCHOR = 0, 1, 2, 3, 4
DEFAULT_MAX, DEFAULT_SLACK = 64, 8
_BASES = b"ACGT"
_CODE = {c: i for i, c in enumerate(b"ACGT")}
_CODE.update({c | 0x20: i for i, c in enumerate(b"ACGT")})


def _b(s):
    return s.encode() if isinstance(s, str) else bytes(s)


def as_set(R):
    return R if isinstance(R, (set, frozenset)) else frozenset(np.asarray(R, np.uint64).tolist())


def _codes(kmer):
    """(forward code, reverse-complement code) of a string of bases, None when a byte is none"""
    f = r = 0
    k = len(kmer)
    for i, c in enumerate(kmer):
        if c not in _CODE:
            return None
        f = (f << 2) | _CODE[c]
        r |= (3 - _CODE[c]) << (2 * i)
    assert f < (1 << (2 * k))
    return f, r


def search(L, Rk, dlo, dhi, budget, k, R):
    R = as_set(R)
    L, Rk = _b(L), _b(Rk)
    assert len(L) == k and len(Rk) == k and 1 <= dlo <= dhi <= MAX_WALK and 1 <= budget <= MAX_BUDGET
    lc, rc = _codes(L), _codes(Rk)
    if lc is None or rc is None:
        return NOANCHOR, 0, b""
    goal = rc[0]
    mask, top = (1 << (2 * k)) - 1, 2 * (k - 1)
    steps, found, first = 1, 0, b""                       # the visit of L: depth 0 < dlo
    stack, path = [[lc[0], lc[1], 0]], []                 # a node: its two codes and the next child to try
    while stack:
        node = stack[-1]
        b = node[2]
        yf = yr = 0
        while b < 4:
            yf, yr = ((node[0] << 2) | b) & mask, (node[1] >> 2) | ((3 - b) << top)
            if min(yf, yr) in R:
                break
            b += 1
        if b == 4:
            stack.pop()
            if path:
                path.pop()
            continue
        node[2] = b + 1
        depth = len(stack)
        steps += 1
        if steps > budget:
            return OVER_BUDGET, steps, b""
        if depth >= dlo and yf == goal:
            found += 1
            if found == 2:
                return AMBIGUOUS, steps, first
            first = bytes(_BASES[x] for x in path + [b])
            continue
        if depth == dhi:
            continue
        stack.append([yf, yr, 0])
        path.append(b)
    return (UNIQUE if found else NONE), steps, first


def query(S, frm, to, dlo, dhi, budget, k, R):
    S, R = _b(S), as_set(R)
    out = {"status": [], "steps": [], "len": [], "walk": []}
    for a, b, lo, hi in zip(frm, to, dlo, dhi):
        a, b = int(a), int(b)
        assert a + k <= len(S) and b + k <= len(S)
        st, steps, walk = search(S[a:a + k], S[b:b + k], int(lo), int(hi), budget, k, R)
        out["status"].append(st); out["steps"].append(steps); out["len"].append(len(walk)); out["walk"].append(walk)
    return out


def sites(S, k, R, M=DEFAULT_MAX):
    S = _b(S)
    ivs = tc.intervals(S, k, R)
    codes = qc._LUT[np.frombuffer(S, dtype=np.uint8)]
    out = []
    for j, (start, end, n) in enumerate(ivs):
        a, b = start - 1, end - k + 1
        d0 = b - a
        if a < 0 or b + k > len(S) or not 2 <= d0 <= M:
            continue
        if np.any(codes[a:a + k] > 3) or np.any(codes[b:b + k] > 3):
            continue
        if j and start - ivs[j - 1][1] < 2:
            continue
        if j + 1 < len(ivs) and ivs[j + 1][0] - end < 2:
            continue
        out.append((start, end, n, a, b, d0))
    return out, len(ivs)


def trim(old, new):
    old, new = _b(old), _b(new)
    uo, un = old.upper(), new.upper()
    p = 0
    while p < len(uo) and p < len(un) and uo[p] == un[p]:
        p += 1
    s = 0
    while s < len(uo) - p and s < len(un) - p and uo[len(uo) - 1 - s] == un[len(un) - 1 - s]:
        s += 1
    return p, old[p:len(old) - s], new[p:len(new) - s]


class Stats:
    def __init__(self):
        self.intervals = self.sites = self.bridged = self.bases_out = self.bases_in = self.ambiguous = self.over_budget = self.removed = 0

    def add(self, o):
        for key in vars(self):
            setattr(self, key, getattr(self, key) + getattr(o, key))

    def tuple(self):
        return (self.intervals, self.sites, self.bridged, self.bases_out, self.bases_in, self.ambiguous, self.over_budget, self.removed)


def bridge(S, k, R, M=DEFAULT_MAX, D=DEFAULT_SLACK, Rs=None):
    """Rs: as_set(R), for a caller that has it"""
    S = _b(S)
    Rs = as_set(R) if Rs is None else Rs
    st = Stats()
    ss, st.intervals = sites(S, k, R, M)
    st.sites = len(ss)
    edits = []
    if not ss:
        return edits, st
    q = query(S, [s[3] for s in ss], [s[4] for s in ss], [max(1, s[5] - D) for s in ss], [s[5] + D for s in ss], BUDGET, k, Rs)
    for i, (start, end, n, a, b, d0) in enumerate(ss):
        if q["status"][i] == AMBIGUOUS:
            st.ambiguous += 1
        if q["status"][i] == OVER_BUDGET:
            st.over_budget += 1
        if q["status"][i] != UNIQUE:
            continue
        old, new = S[a:b + k], S[a:a + k] + q["walk"][i]
        p, ref, alt = trim(old, new)
        assert p >= k and (ref or alt)
        edits.append((a + p, ref.decode() or ".", alt.decode() or ".", n, q["steps"][i]))
        st.bridged += 1
        st.bases_out += len(ref)
        st.bases_in += len(alt)
        st.removed += n
    assert edits == sorted(edits) and all(x[0] + (len(x[1]) if x[1] != "." else 0) <= y[0] for x, y in zip(edits, edits[1:]))
    return edits, st


def apply(S, edits):
    """positions are those of S: the edits go in from the last to the first"""
    S = bytearray(_b(S))
    for pos, ref, alt, _, _ in sorted(edits, reverse=True):
        ref, alt = ("" if x == "." else x for x in (ref, alt))
        assert S[pos:pos + len(ref)] == ref.encode()
        S[pos:pos + len(ref)] = alt.encode()
    return bytes(S)


def run(contigs, k, R, M=DEFAULT_MAX, D=DEFAULT_SLACK):
    lines, out, st = [HEADER], [], Stats()
    Rs = as_set(R)
    for name, S in contigs:
        edits, s = bridge(S, k, R, M, D, Rs)
        st.add(s)
        out.append((name, apply(S, edits).decode()))
        lines += [f"{name}\t{pos}\t{ref}\t{alt}\t{n}\t{steps}" for pos, ref, alt, n, steps in edits]
    return out, "\n".join(lines) + "\n", st


def parse_tsv(text):
    lines = text.split("\n")
    assert lines[0] == HEADER and lines[-1] == ""
    out = []
    for l in lines[1:-1]:
        f = l.split("\t")
        assert len(f) == 6, l
        out.append((f[0], int(f[1]), f[2], f[3], int(f[4]), int(f[5])))
    return out


def info_line(path, k, M, D, st):
    return (f"[Hypo::Hypo] Info: k-mer bridge {path} (k = {k}, max {M}, slack {D}): {st.intervals} intervals, {st.sites} sites, {st.bridged} bridged "
            f"({st.bases_out} bases out, {st.bases_in} bases in), {st.ambiguous} ambiguous, {st.over_budget} over budget, {st.removed} missing k-mers removed")
