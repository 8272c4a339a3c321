"""CPU checker of `hypo --kmer-bridge-vote` and hypo_gpu_kset_query_walk_sets (DESIGN.md "k-mer bridge vote"): the contract in plain
Python on top of kmer_bridge_checker and min_count_checker.  It shares no code with the host library or the kernels.

C maps a canonical code to the number of windows of the reads that have it, stopping at 255 (count_map); count(y) is C's value for
y's canonical code, 0 when absent; t is the least count in force.  With W = 4 the WALKS of a query (L, Rk, dlo, dhi, budget) are what
this search finds, and its answer is the search's and nothing else:

    steps = 0; walks = []
    visit(x, depth, path, lo):
        steps += 1;  if steps > budget: stop with BUDGET
        if depth >= dlo and x == Rk:
            if len(walks) == W: stop with MANY
            walks.append((path, lo));  return
        if depth == dhi: return
        for b in A, C, G, T:  y = x[1:] + b;  c = count(y);  if c >= t: visit(y, depth + 1, path + b, min(lo, c))
    visit(L, 0, "", 255)
    status = NONE / UNIQUE / AMBIGUOUS for 0 / 1 / 2..W walks

BUDGET (steps = budget + 1) and NOANCHOR (steps 0) report no walk, MANY the first W.

The vote: the sites of kmer_bridge_checker whose query ends AMBIGUOUS are asked again with this search (the same from, to, dlo, dhi,
budget 4096).  A site is CHOSEN when the second search ends AMBIGUOUS and the largest low c1 and the second largest c2 of its walks
satisfy c1 >= ratio * c2; the walk with c1 is then edited in as a unique site's is, with the second search's steps.  Every other
asked site is left alone and counted: too close, more than W walks, over budget.  The TSV gains the columns walks and support: 1 and
"." for a unique bridge, the number of walks and c1/c2 for a chosen one.

  count_map(keys, counts)                                 C of min_count_checker.read_counts' arrays
  read_count_map(paths_or_seqs, k)                        C of reads files or byte strings
  search_set(L, Rk, dlo, dhi, budget, k, C, t)            (status, steps, [(walk bytes, low)]) of one query
  query_sets(S, frm, to, dlo, dhi, budget, k, C, t)       what the entry point answers: dict of status, steps, n_walks and walks (lists)
  decide(walks, ratio)                                    (index of the chosen walk or None, c1, c2) for the walks of an AMBIGUOUS answer
  bridge_vote(S, k, C, t, ratio, M, D)                    (edits [(pos, ref, alt, n, steps, walks, support)] ascending, Stats, Vote) of one contig
  run(contigs, k, C, t, ratio, M, D)                      ([(name, new text)], the TSV's text, Stats, Vote) for [(name, S)] in draft order
  parse_tsv(text)                                         [(contig, pos, ref, alt, n, steps, walks, support)]
  info_lines(path, k, M, D, ratio, stats, vote)           the two lines stdout gains
"""
import numpy as np

import kmer_bridge_checker as kb
import min_count_checker as mc

HEADER = kb.HEADER + "\twalks\tsupport"
W = 4
MANY = 5
CAP = 255
_BASES = b"ACGT"


def count_map(keys, counts):
    return {int(key): min(int(c), CAP) for key, c in zip(keys, counts)}


def read_count_map(paths_or_seqs, k):
    return count_map(*mc.read_counts(paths_or_seqs, k))


def search_set(L, Rk, dlo, dhi, budget, k, C, t=1):
    L, Rk = kb._b(L), kb._b(Rk)
    assert len(L) == k and len(Rk) == k and 1 <= dlo <= dhi <= kb.MAX_WALK and 1 <= budget <= kb.MAX_BUDGET and 1 <= t <= CAP
    lc, rc = kb._codes(L), kb._codes(Rk)
    if lc is None or rc is None:
        return kb.NOANCHOR, 0, []
    goal = rc[0]
    mask, top = (1 << (2 * k)) - 1, 2 * (k - 1)
    steps, walks = 1, []                                  # the visit of L: depth 0 < dlo
    stack, path = [[lc[0], lc[1], 0, CAP]], []            # a node: its two codes, the next child to try, the least count down to it
    while stack:
        node = stack[-1]
        b = node[2]
        yf = yr = c = 0
        while b < 4:
            yf, yr = ((node[0] << 2) | b) & mask, (node[1] >> 2) | ((3 - b) << top)
            c = C.get(min(yf, yr), 0)
            if c >= t:
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
            return kb.OVER_BUDGET, steps, []
        if depth >= dlo and yf == goal:
            if len(walks) == W:
                return MANY, steps, walks
            walks.append((bytes(_BASES[x] for x in path + [b]), min(node[3], c)))
            continue
        if depth == dhi:
            continue
        stack.append([yf, yr, 0, min(node[3], c)])
        path.append(b)
    return (kb.NONE, kb.UNIQUE, kb.AMBIGUOUS)[min(len(walks), 2)], steps, walks


def query_sets(S, frm, to, dlo, dhi, budget, k, C, t=1):
    S = kb._b(S)
    out = {"status": [], "steps": [], "n_walks": [], "walks": []}
    for a, b, lo, hi in zip(frm, to, dlo, dhi):
        a, b = int(a), int(b)
        assert a + k <= len(S) and b + k <= len(S)
        st, steps, walks = search_set(S[a:a + k], S[b:b + k], int(lo), int(hi), budget, k, C, t)
        out["status"].append(st); out["steps"].append(steps); out["n_walks"].append(len(walks)); out["walks"].append(walks)
    return out


def decide(walks, ratio):
    """walks: [(bytes, low)] of an AMBIGUOUS answer (2..W of them).  The walks sorted by low, largest first: c1, c2 are the first two;
    chosen iff c1 >= ratio * c2, and then c1 > c2, so the walk with c1 is one walk."""
    assert 2 <= len(walks) <= W and 2 <= ratio <= CAP
    order = sorted(range(len(walks)), key=lambda i: -walks[i][1])
    c1, c2 = walks[order[0]][1], walks[order[1]][1]
    return (order[0] if c1 >= ratio * c2 else None), c1, c2


class Vote:
    def __init__(self):
        self.asked = self.chosen = self.close = self.many = self.over_budget = 0

    def add(self, o):
        for key in vars(self):
            setattr(self, key, getattr(self, key) + getattr(o, key))

    def tuple(self):
        return (self.asked, self.chosen, self.close, self.many, self.over_budget)


def reliable(C, t):
    """the codes counted at least t times: (as a sorted array, as a set)"""
    R = np.array(sorted(key for key, c in C.items() if c >= t), np.uint64)
    return R, kb.as_set(R)


def bridge_vote(S, k, C, t, ratio, M=kb.DEFAULT_MAX, D=kb.DEFAULT_SLACK, Rt=None):
    """Rt: reliable(C, t), for a caller that has it"""
    S = kb._b(S)
    R, Rs = reliable(C, t) if Rt is None else Rt
    st, vt = kb.Stats(), Vote()
    ss, st.intervals = kb.sites(S, k, R, M)
    st.sites = len(ss)
    edits = []
    for start, end, n, a, b, d0 in ss:
        dlo, dhi = max(1, d0 - D), d0 + D
        status, steps, walk = kb.search(S[a:a + k], S[b:b + k], dlo, dhi, kb.BUDGET, k, Rs)
        n_walks, support = 1, "."
        if status == kb.OVER_BUDGET:
            st.over_budget += 1
        if status == kb.AMBIGUOUS:
            vt.asked += 1
            status2, steps, walks = search_set(S[a:a + k], S[b:b + k], dlo, dhi, kb.BUDGET, k, C, t)
            pick = None
            if status2 == MANY:
                vt.many += 1
            elif status2 == kb.OVER_BUDGET:
                vt.over_budget += 1
            else:
                assert status2 == kb.AMBIGUOUS
                pick, c1, c2 = decide(walks, ratio)
                if pick is None:
                    vt.close += 1
            if pick is None:
                st.ambiguous += 1
                continue
            vt.chosen += 1
            walk, n_walks, support = walks[pick][0], len(walks), f"{c1}/{c2}"
        elif status != kb.UNIQUE:
            continue
        old, new = S[a:b + k], S[a:a + k] + walk
        p, ref, alt = kb.trim(old, new)
        assert p >= k and (ref or alt)
        edits.append((a + p, ref.decode() or ".", alt.decode() or ".", n, steps, n_walks, support))
        st.bridged += 1
        st.bases_out += len(ref)
        st.bases_in += len(alt)
        st.removed += n
    assert edits == sorted(edits) and all(x[0] + (len(x[1]) if x[1] != "." else 0) <= y[0] for x, y in zip(edits, edits[1:]))
    assert vt.asked == vt.chosen + vt.close + vt.many + vt.over_budget
    return edits, st, vt


def run(contigs, k, C, t, ratio, M=kb.DEFAULT_MAX, D=kb.DEFAULT_SLACK):
    lines, out, st, vt = [HEADER], [], kb.Stats(), Vote()
    Rt = reliable(C, t)
    for name, S in contigs:
        edits, s, v = bridge_vote(S, k, C, t, ratio, M, D, Rt)
        st.add(s)
        vt.add(v)
        out.append((name, kb.apply(S, [e[:5] for e in edits]).decode()))
        lines += [f"{name}\t" + "\t".join(str(x) for x in e) for e in edits]
    return out, "\n".join(lines) + "\n", st, vt


def parse_tsv(text):
    lines = text.split("\n")
    assert lines[0] == HEADER and lines[-1] == ""
    out = []
    for l in lines[1:-1]:
        f = l.split("\t")
        assert len(f) == 8, l
        out.append((f[0], int(f[1]), f[2], f[3], int(f[4]), int(f[5]), int(f[6]), f[7]))
    return out


def info_lines(path, k, M, D, ratio, st, vt):
    return [kb.info_line(path, k, M, D, st),
            f"[Hypo::Hypo] Info: k-mer bridge vote (ratio {ratio}, up to {W} walks): {vt.asked} asked, {vt.chosen} chosen, {vt.close} too close, "
            f"{vt.many} more than {W} walks, {vt.over_budget} over budget"]
