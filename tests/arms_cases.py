"""The inputs of the direct tests of arm selection (tests/test_arms_checker_cpu.py on the host loops, tests/test_gpu_arms_direct.py on
the kernels of arms_kernel.hip): region tables and reads as the flat arrays of HypoArmsRegions / HypoArmsReads, built by hand so that
they reach what simulated reads almost never do — CIGAR operations that end on a border, every outcome of the four anchor searches,
both sides of every pruning threshold, a file order that is not the position order, odd packing offsets, more than 1024 and more
than 1024 x 1024 items in the prefix sums — and, for every case, the condition that makes it worth running, computed from the inputs
and the trace of tests/arms_checker.py alone.

A case is built once per process, and so is what the checker says about it (expected)."""
import functools
from collections import Counter, namedtuple

import numpy as np

import arms_checker as ac
from arms_checker import SWS, SW, WS, MWM, MW, WM, SWM, MWS, OTHER, LONG, SR, MSR, INTERNAL, PREFIX, SUFFIX

Regions = namedtuple("Regions", "n_regions start type info n_anchor_kmers anchor_kmers k contig4 codes")
Reads = namedtuple("Reads", "rb re qae seq_off reads2 reads2_bytes cigar_off cigar file_rank")
Case = namedtuple("Case", "name long_mode regions reads notes")

OPS = {"M": 0, "I": 1, "D": 2, "N": 3, "S": 4, "H": 5, "P": 6, "=": 7, "X": 8}
S_LEFT, S_RIGHT, M_LEFT, M_RIGHT = (SWS, SW, SWM), (SWS, WS, MWS), (MWM, MW, MWS), (MWM, WM, SWM)


# ---- building blocks -------------------------------------------------------------------------------------------------------------

def rand_codes(rng, n):
    return rng.integers(0, 4, size=n, dtype=np.uint8)


def pack4(codes):
    c = np.concatenate([codes, np.zeros(codes.size % 2, np.uint8)]).reshape(-1, 2)
    return ((c[:, 0] << 4) | c[:, 1]).astype(np.uint8)


def kmer_at(codes, p, k):
    v = 0
    for b in codes[p:p + k].tolist():
        v = (v << 2) | b
    return v


def make_regions(codes, layout, k, long_mode=False):
    """layout: [(start, type)] in order, the first at 0.  The end marker (the total length, OTHER) is appended; info and the anchor
    k-mers are read off the contig: an SR of k or more bases gets the next rank and its first / last k-mer, a shorter one (a filler
    between contigs) rank 0; an MSR gets the 10-mer at its start."""
    n = len(layout)
    start = np.array([s for s, _ in layout] + [codes.size], dtype=np.uint32)
    rtype = np.array([t for _, t in layout] + [OTHER], dtype=np.uint8)
    info = np.zeros(n + 1, dtype=np.uint32)
    anchors = [0]
    if not long_mode:
        for i, (s, t) in enumerate(layout):
            e = int(start[i + 1])
            if t == SR and e - s >= k:
                info[i] = (len(anchors) + 1) // 2
                anchors += [kmer_at(codes, s, k), kmer_at(codes, e - k, k)]
            elif t == MSR:
                info[i] = kmer_at(codes, s, ac.MK)
    a = np.array(anchors, dtype=np.uint64)
    return Regions(n, start, rtype, info, a.size, a, k, pack4(codes), codes)


def make_read(codes, rb, ops, rng):
    """ops: [(op letter, length)] or (op letter, length, bases) -> (rb, re, query bases, cigar words).  M and = copy the contig, X copies it
    with every base changed, I takes random bases (or the ones given), D and N skip, S and H only appear in the CIGAR (the arrays hold
    the aligned part of the query)."""
    q, cigar, pos = [], [], rb
    for op in ops:
        o, n = op[0], op[1]
        assert n > 0, ops
        cigar.append((n << 4) | OPS[o])
        if o in "M=":
            q += codes[pos:pos + n].tolist(); pos += n
        elif o == "X":
            q += [(int(b) + 1 + int(rng.integers(0, 3))) % 4 for b in codes[pos:pos + n]]; pos += n
        elif o == "I":
            q += list(op[2]) if len(op) > 2 else rng.integers(0, 4, size=n).tolist()
        elif o in "DN":
            pos += n
    assert pos <= codes.size, (rb, ops)
    return rb, pos, q, cigar


def exact(codes, rb, re):
    return rb, re, codes[rb:re].tolist(), [((re - rb) << 4) | 0]


def pack_reads(recs, file_rank=None, odd_offsets=False):
    """recs: [(rb, re, query bases, cigar words)] in FILE order -> Reads sorted by rb (a stable sort), every read packed four bases to a
    byte from its own byte offset.  file_rank: "keep" records where every read stood in recs; None leaves it out (the sorted order is
    then the file order).  odd_offsets: a spare byte goes in front of a read whenever its offset would be even."""
    order = sorted(range(len(recs)), key=lambda i: recs[i][0])
    n = len(recs)
    rb = np.array([recs[i][0] for i in order], dtype=np.uint32)
    re = np.array([recs[i][1] for i in order], dtype=np.uint32)
    qae = np.array([len(recs[i][2]) for i in order], dtype=np.uint32)
    seq_off = np.zeros(n, dtype=np.uint64)
    cigar_off = np.zeros(n + 1, dtype=np.uint32)
    chunks, cig, at = [], [], 0
    for j, i in enumerate(order):
        q = recs[i][2]
        if odd_offsets and at % 2 == 0:
            chunks.append(np.full(1, 0xA5, dtype=np.uint8)); at += 1
        c = np.concatenate([np.array(q, dtype=np.uint8), np.zeros((-len(q)) % 4, np.uint8)]).reshape(-1, 4)
        chunks.append(((c[:, 0] << 6) | (c[:, 1] << 4) | (c[:, 2] << 2) | c[:, 3]).astype(np.uint8))
        seq_off[j] = at
        at += c.shape[0]
        cig += recs[i][3]
        cigar_off[j + 1] = len(cig)
    chunks.append(np.zeros(4, dtype=np.uint8))
    reads2 = np.concatenate(chunks)
    rank = np.array(order, dtype=np.uint32) if file_rank == "keep" else None
    return Reads(rb, re, qae, seq_off, reads2, reads2.size, cigar_off, np.array(cig, dtype=np.uint32), rank)


def check_tables(case):
    """What hypo_gpu_arms_build does not check and the kernels rely on.  A case that fails here is a bug in the case: it never
    reaches the library.  (An SR that no window's type points at may carry rank 0: the 1-base filler between two contigs.)"""
    R, A = case.regions, case.reads
    n = R.n_regions
    start, rtype, info = R.start.astype(np.int64), R.type, R.info
    assert start.size == n + 1 and rtype.size == n + 1 and start[0] == 0 and (np.diff(start) > 0).all(), "starts"
    assert start[n] == R.codes.size and R.contig4.size == (R.codes.size + 1) // 2, "end marker / contig"
    assert not ac.is_sr(int(rtype[n])), "the end marker is an SR"
    if case.long_mode:
        assert all(int(t) in (SR, LONG) for t in rtype[:n]), "pseudo regions are SR or LONG"
    else:
        assert info.size == n + 1 and R.anchor_kmers.size == R.n_anchor_kmers
        assert not (rtype[:n] == LONG).any()
        for w in np.nonzero((rtype[:n] != OTHER))[0].tolist():
            t = int(rtype[w])
            if t in S_LEFT or t in M_LEFT:
                assert w >= 1 and int(rtype[w - 1]) == (SR if t in S_LEFT else MSR), f"region {w}: nothing to anchor on at its left"
            if t in S_RIGHT or t in M_RIGHT:
                assert w + 1 < n and int(rtype[w + 1]) == (SR if t in S_RIGHT else MSR), f"region {w}: nothing to anchor on at its right"
            for nb, pointed in ((w - 1, t in S_LEFT), (w + 1, t in S_RIGHT)):
                if pointed:
                    assert 1 <= int(info[nb]), f"region {nb}: an SR a window anchors on has rank 0"
            if t == SR:
                r = int(info[w])
                assert 2 * r < R.n_anchor_kmers or r == 0, f"region {w}: rank {r} beyond the anchor k-mers"
                if r:
                    s, e = int(start[w]), int(start[w + 1])
                    assert e - s >= R.k and int(R.anchor_kmers[2 * r - 1]) == kmer_at(R.codes, s, R.k) and int(R.anchor_kmers[2 * r]) == kmer_at(R.codes, e - R.k, R.k), f"region {w}: anchors"
            if t == MSR:
                assert int(start[w]) + ac.MK <= R.codes.size and int(info[w]) == kmer_at(R.codes, int(start[w]), ac.MK), f"region {w}: minimizer"
    m = A.rb.size
    assert A.re.size == m and A.qae.size == m and A.seq_off.size == m and A.cigar_off.size == m + 1 and A.reads2_bytes == A.reads2.size
    if A.file_rank is not None:
        assert sorted(A.file_rank.tolist()) == list(range(m)), "file_rank is no permutation"
    for a in range(m):
        qsum = rsum = 0
        for c in A.cigar[int(A.cigar_off[a]):int(A.cigar_off[a + 1])].tolist():
            t = ac.CIGAR_TYPE[c & 15]
            if (c & 15) in (4, 5):
                continue
            qsum += (c >> 4) if t & 1 else 0
            rsum += (c >> 4) if t & 2 else 0
        rb, re = int(A.rb[a]), int(A.re[a])
        assert qsum == int(A.qae[a]) and rsum == re - rb and re > rb and re <= int(start[n]) and (a == 0 or int(A.rb[a - 1]) <= rb), f"alignment {a}"
        assert int(A.seq_off[a]) + (int(A.qae[a]) + 3) // 4 <= A.reads2_bytes, f"alignment {a}: bases beyond reads2"
    # (the device leaves one record of more than 16 384 bases and more than 64 x the mean span to the host)
    span = A.re.astype(np.int64) - A.rb
    assert m == 0 or not (span.max() > 16384 and span.max() * m > 64 * span.sum())


def tiled_layout(rng, n_units, k, win_len, sr_len=None):
    """the twelve region types in an order in which every window has the neighbours its type names, repeated:
    SR SWS SR SWM MSR MWM MSR MWS SR SW OTHER WM MSR MW WS | SR ..."""
    unit = [SR, SWS, SR, SWM, MSR, MWM, MSR, MWS, SR, SW, OTHER, WM, MSR, MW, WS]
    layout, at = [], 0
    for _ in range(n_units):
        for t in unit:
            layout.append((at, t))
            at += (sr_len or 2 * k + 8) if t == SR else ac.MK if t == MSR else int(win_len(rng))
    layout.append((at, SR))
    at += sr_len or 2 * k + 8
    return layout, at


# ---- short mode --------------------------------------------------------------------------------------------------------------------

def _corners():
    rng = np.random.default_rng(101)
    k = 13
    layout, total = tiled_layout(rng, 6, k, lambda r: r.integers(18, 40))
    # in every other unit the windows name no SR: nothing re-anchors an arm there, so a break point next to an SR shows as it was decided
    plain = {SWS: OTHER, SW: OTHER, WS: OTHER, SWM: WM, MWS: MW}
    layout = [(s, plain.get(t, t) if (i // 15) % 2 else t) for i, (s, t) in enumerate(layout)]
    codes = rand_codes(rng, total)
    R = make_regions(codes, layout, k)
    borders = R.start.tolist()
    recs = []
    for n in range(420):
        span = int(rng.integers(60, 260))
        rb = int(rng.integers(0, total - span))
        re = rb + span
        if n % 5 == 0:                                          # begins on a border
            rb = borders[int(np.searchsorted(R.start, rb))]
        if n % 7 == 0:                                          # ends on one
            re = borders[int(np.searchsorted(R.start, re))]
        if n % 9 == 0:                                          # lies inside one region
            i = int(rng.integers(0, R.n_regions))
            if borders[i + 1] - borders[i] >= 14:
                rb, re = borders[i] + 1, borders[i + 1] - 1
        if re - rb < 8:
            continue
        ops, pos = [], rb
        if rng.integers(0, 3) == 0:
            ops.append(("H", 3))
        if rng.integers(0, 3) == 0:
            ops.append(("S", int(rng.integers(1, 9))))
        if rng.integers(0, 8) == 0:
            ops.append(("I", 2))                              # an insertion in front of the first aligned base
        for b in [x for x in borders if rb < x < re]:
            style = int(rng.integers(0, 6))
            if style == 0 or b - pos < 4 or re - b < 6:
                continue                                       # the border falls inside an operation
            end_kind = "M=XDN"[int(rng.integers(0, 5))]
            if end_kind in "DN":                               # a deletion that ends on the border
                d = int(rng.integers(1, 3))
                ops += [("M=X"[int(rng.integers(0, 3))], b - pos - d), (end_kind, d)]
            else:
                ops.append((end_kind, b - pos))
            pos = b
            if style in (1, 2):
                pass                                           # ... then M / = / X
            elif style == 3:                                   # ... then D / N
                d = int(rng.integers(1, 3))
                ops.append(("DN"[int(rng.integers(0, 2))], d)); pos += d
            else:                                              # ... then an insertion
                ops.append(("I", int(rng.integers(1, 4))))
        if re > pos:
            ops.append(("M=X"[int(rng.integers(0, 3))], re - pos))
        if rng.integers(0, 8) == 0:
            ops.append(("I", 1))                              # ... and behind the last one
        if rng.integers(0, 3) == 0:
            ops.append(("S", int(rng.integers(1, 9))))
        recs.append(make_read(codes, rb, ops, rng))
    return Case("corners", False, R, pack_reads(recs), {})


def _corners_condition(c, x):
    t = x.trace
    for how in ("inside", "corner_M", "corner_DN", "corner_I_sr", "corner_I_win"):
        assert t["bp"][how] >= 20, (how, t["bp"])
    assert t["first"][INTERNAL] >= 20 and t["first"][SUFFIX] >= 20 and t["last"][INTERNAL] >= 20 and t["last"][PREFIX] >= 20, (t["first"], t["last"])
    assert t["single_region"] >= 20, t["single_region"]
    # an insertion on a border with an SR or MSR on its left, in front of a window that does not re-anchor its left end
    R = c.regions
    bare = sum(1 for w in range(1, R.n_regions) if ac.is_sr(int(R.type[w - 1])) and int(R.type[w]) in (OTHER, WM, WS))
    assert bare >= 6, bare
    return dict(bp=dict(t["bp"]), first=dict(t["first"]), last=dict(t["last"]), single_region=t["single_region"])


def _empty_arms():
    rng = np.random.default_rng(102)
    k = 13
    # OTHER windows of 24 bases, an SR every eighth region
    layout, at = [], 0
    for i in range(64):
        sr = i % 8 == 0
        layout.append((at, SR if sr else OTHER))
        at += 40 if sr else 24
    codes = rand_codes(rng, at)
    R = make_regions(codes, layout, k)
    st = R.start.tolist()
    recs = []
    # region 3: one read over it and three reads that delete it whole: valid only because the empty arms count as internal
    recs.append(exact(codes, st[2] + 3, st[4] + 9))
    for j in range(3):
        recs.append(make_read(codes, st[2] + 2 + j, [("M", st[3] - st[2] - 6 - j), ("D", st[4] - st[3] + 9), ("M", 20 + j)], rng))
    # reads with a D over one, two or three whole windows (never region 3 again)
    for n in range(60):
        first = int(rng.integers(9, 58))
        m = int(rng.integers(1, 4))
        if any(layout[i][1] == SR for i in range(first - 1, first + m + 1)):
            continue
        lead, tail = int(rng.integers(8, 22)), int(rng.integers(8, 22))
        x = st[first] - int(rng.integers(0, 4))               # the deletion begins on the border or up to three bases in front of it
        y = st[first + m] + int(rng.integers(0, 4))
        recs.append(make_read(codes, x - lead, [("M", lead), ("DN"[n % 2], y - x), ("M", tail)], rng))
    for n in range(120):
        span = int(rng.integers(60, 160))
        rb = int(rng.integers(st[8], at - span))
        recs.append(exact(codes, rb, rb + span))
    return Case("empty_arms", False, R, pack_reads(recs), {})


def _empty_arms_condition(c, x):
    wins = x.trace["windows"]
    n_empty = sum(w["n_empty"] for w in wins.values())
    saved = [i for i, w in wins.items() if w["valid"] and w["internal"] >= ac.MIN_SHORT_NUM and w["n_int"] < ac.MIN_SHORT_NUM and (w["n_pre"] < 3 or w["n_suf"] < 3)]
    assert n_empty >= 30 and 3 in saved, (n_empty, saved)
    return dict(empty_arms=n_empty, windows_valid_by_their_empty_arms=len(saved))


def _anchors(k, seed):
    rng = np.random.default_rng(seed)
    wl = lambda r: [20, 24, 30, 40, 50, 60, 47, 53][int(r.integers(0, 8))] if k < 31 else [40, 50, 60, 70, 47, 53, 20, 30][int(r.integers(0, 8))]
    sr_len = 3 * k + 4
    layout, total = tiled_layout(rng, 5, k, wl, sr_len)
    codes = rand_codes(rng, total)
    start = [s for s, _ in layout] + [total]
    types = [t for _, t in layout]
    # the draft holds an anchor a second time inside the search range: every other SR ends / begins with its k-mer twice, every other
    # minimizer stands again at the start of the window behind it or at the end of the window in front of it
    for i, t in enumerate(types):
        s, e = start[i], start[i + 1]
        if t == SR and i % 4 == 0:
            codes[e - 2 * k:e - k] = codes[e - k:e]
        if t == SR and i % 4 == 2:
            codes[s + k:s + 2 * k] = codes[s:s + k]
    for i, t in enumerate(types):
        s, e = start[i], start[i + 1]
        if t == MSR and i % 2 == 0 and start[i + 2] - e >= 20:
            codes[e:e + 10] = codes[s:s + 10]
        if t == MSR and i % 2 == 1 and s - start[i - 1] >= 20:
            codes[s - 10:s] = codes[s:s + 10]
    R = make_regions(codes, layout, k)
    recs = []
    wins = [i for i, t in enumerate(types) if not ac.is_sr(t)]
    for n in range(1500):
        w = wins[int(rng.integers(0, len(wins)))]
        t = types[w]
        ws, we = start[w], start[w + 1]
        lk = k if t in S_LEFT else ac.MK                         # the length of the anchor on either side (OTHER, SW, ...: as if 10)
        rk = k if t in S_RIGHT else ac.MK

        def recipe(kk, far):
            """(bases of the read beyond the border, shift of the CIGAR at the border, spoil the anchor)"""
            what = int(rng.integers(0, 8))
            if what == 0:
                return int(rng.integers(0, kk)), 0, False                      # too close to the read's end
            ext = int(rng.integers(kk + 5, far + 6)) if what in (1, 2) else int(rng.integers(far + 6, far + 14))    # (1, 2: the range is clamped at the read's end)
            if what in (1, 3, 4):
                return ext, int(rng.integers(1, 5)) * (1 if rng.integers(0, 2) else -1), False
            if what in (2, 5):
                return ext, 0, True
            return ext, 0, False

        lext, ls, lmut = recipe(lk, 2 * k if t in S_LEFT else 3 * ac.MK)
        rext, rs, rmut = recipe(rk, 2 * k if t in S_RIGHT else 3 * ac.MK)
        short = int(rng.integers(0, 12))
        if short == 0:                                          # the read ends a few bases into the window / begins a few before its end
            rext, rs, rmut = -(we - ws) + int(rng.integers(1, 8)), 0, False
        elif short == 1:
            lext, ls, lmut = -(we - ws) + int(rng.integers(1, 8)), 0, False
        rb, re = ws - lext, we + rext
        if rb < 0 or re > total or re - rb < 12:
            continue
        q = codes[rb:re].tolist()
        if lmut and lext >= 3:
            q[lext - 2] = (q[lext - 2] + 1) % 4
        if rmut and rext >= 3:
            q[(we - rb) + 1] = (q[(we - rb) + 1] + 2) % 4
        # the CIGAR describes the copy with a deletion and an insertion of the same size either side of a border: the bases between the
        # two stand |shift| away from where the CIGAR puts them
        cuts = []                                             # (reference position, op, length)
        wlen = we - ws
        if ls and lext > abs(ls) + 4 and wlen >= 18 and lext >= 0:
            cuts += [(ws - 2 - (abs(ls) if ls < 0 else 0), "D" if ls < 0 else "I", abs(ls)), (ws + 2, "I" if ls < 0 else "D", abs(ls))]
        if rs and rext > abs(rs) + 4 and wlen >= 18 and rext >= 0 and lext > -(wlen - 12):
            cuts += [(we - 2 - (abs(rs) if rs < 0 else 0), "D" if rs < 0 else "I", abs(rs)), (we + 2, "I" if rs < 0 else "D", abs(rs))]
        ops, pos = [], rb
        for p, o, ln in cuts:
            if p <= pos:
                ops = None
                break
            ops.append(("M", p - pos)); pos = p
            ops.append((o, ln))
            if o == "D":
                pos += ln
        if ops is None or pos >= re:
            continue
        ops.append(("M", re - pos))
        cigar = [(ln << 4) | OPS[o] for o, ln in ops]
        recs.append((rb, re, q, cigar))
    # the anchor is found d bases further in and the prefix arm is d bases long: nothing is left of it.  The read is a copy of
    # [rb, re - d); the CIGAR deletes d bases in front of the border, so that what it calls the border stands d bases early
    for n in range(60):
        w = wins[int(rng.integers(0, len(wins)))]
        t, ws, wlen = types[w], start[w], start[w + 1] - start[w]
        d = 2 if wlen <= 20 else 3
        if not (t in S_LEFT or t in M_LEFT) or wlen > 10 * d:
            continue
        far = 2 * k if t in S_LEFT else 3 * ac.MK
        rb, re = ws - far - 8, ws + d
        recs.append((rb, re, codes[rb:re - d].tolist(), [((ws - 2 - d - rb) << 4) | 0, (d << 4) | 2, ((2 + d) << 4) | 0]))
    return Case(f"anchors_k{k}", False, R, pack_reads(recs), {})


def _anchors_condition(c, x):
    cells, two, clamp0, clampq = Counter(), Counter(), 0, 0
    coef = exact_coef = crossed = 0
    for r in x.trace["arms"]:
        coef += r["result"] == "coef"
        exact_coef += r["result"] != "coef" and r["coef_margin"] == 0
        crossed += r["result"] == "crossed"
        for side in ("LS", "RS", "LM", "RM"):
            s = r.get(side)
            if s:
                cells[side, s["outcome"]] += 1
                two[side[0]] += s["hits"] >= 2
                clamp0 += s["clamp0"]; clampq += s["clampq"]
    for side in ("LS", "RS", "LM", "RM"):
        for outcome in ("exact", "moved", "notfound", "edge"):
            assert cells[side, outcome] >= 10, (side, outcome, sorted(cells.items()))
    assert two["L"] >= 10 and two["R"] >= 10 and clamp0 >= 10 and clampq >= 10, (two, clamp0, clampq)
    assert coef >= 10 and exact_coef >= 10 and crossed >= 5, (coef, exact_coef, crossed)
    seen = set(int(t) for t in c.regions.type[:c.regions.n_regions])
    assert seen == set(range(12)) - {LONG}
    return dict(searches={f"{s}:{o}": n for (s, o), n in sorted(cells.items())}, two_hits=dict(two), clamped_at_0=clamp0, clamped_at_qae=clampq,
                refused_by_coef=coef, coef_exact=exact_coef, crossed=crossed)


PRUNING_PAIRS = [
    # (name, type, (internal, prefix, suffix, longest prefix, longest suffix) of either window; lengths None: 30 + 30 of 50)
    ("internal_2_3", OTHER, (2, 1, 1), (3, 1, 1)),
    ("prefix_2_3", OTHER, (0, 2, 3), (0, 3, 3)),
    ("suffix_2_3", OTHER, (1, 3, 2), (1, 3, 3)),
    ("covered", OTHER, (0, 3, 3, 30, 19), (0, 3, 3, 30, 20)),
    ("covered_mwm", MWM, (2, 3, 3, 24, 25), (2, 3, 3, 25, 25)),
    ("internal_20_21", OTHER, (20, 17, 17), (21, 17, 17)),
    ("internal_20_21_mw", MW, (20, 17, 17), (21, 17, 17)),
    ("contrib_9_10", OTHER, (4, 3, 2), (4, 3, 3)),
    ("floor", OTHER, (3, 4, 3), (4, 4, 3)),
    ("floor_wm", WM, (4, 5, 4), (5, 5, 4)),
    ("s_4_5_sws", SWS, (4, 2, 2), (5, 2, 2)),
    ("s_4_5_sw", SW, (4, 2, 2), (5, 2, 2)),
    ("s_4_5_ws", WS, (4, 2, 2), (5, 2, 2)),
    ("s_4_5_mws", MWS, (4, 2, 2), (5, 2, 2)),
    ("s_4_5_swm", SWM, (4, 2, 2), (5, 2, 2)),
    ("other_5_6", OTHER, (5, 2, 2), (6, 2, 2)),
    ("mwm_5_6", MWM, (5, 2, 2), (6, 2, 2)),
]


def _isolated_windows(rng, specs, k, win_len=50):
    """one window per spec (its type), every one between what its type names and SRs beyond: a read of 20 bases either side of the window
    touches no other window.  -> (layout, total, [region index of the window])"""
    layout, at, idx = [(0, SR)], 40, []
    for t in specs:
        if t in M_LEFT:
            layout.append((at, MSR)); at += ac.MK
        idx.append(len(layout))
        layout.append((at, t)); at += win_len(rng) if callable(win_len) else win_len
        if t in M_RIGHT:
            layout.append((at, MSR)); at += ac.MK
        layout.append((at, SR)); at += 40
    return layout, at, idx


def _window_reads(codes, ws, we, n_int, n_pre, n_suf, max_pre=None, max_suf=None, rng=None):
    """exact copies: n_int over the whole window, n_pre that end inside it (the longest max_pre bases in), n_suf that begin inside it"""
    recs = []
    for j in range(n_int):
        recs.append(exact(codes, ws - 20 - j % 5, we + 20 + j % 3))
    for j in range(n_pre):
        recs.append(exact(codes, ws - 20 - j % 4, ws + (max_pre or 30) - j % 3 * (j > 0)))
    for j in range(n_suf):
        recs.append(exact(codes, we - (max_suf or 30) + j % 3 * (j > 0), we + 20 + j % 4))
    return recs


def _pruning():
    rng = np.random.default_rng(104)
    k = 13
    specs = [t for _, t, _, _ in PRUNING_PAIRS for _ in range(2)]
    layout, total, idx = _isolated_windows(rng, specs, k)
    codes = rand_codes(rng, total)
    R = make_regions(codes, layout, k)
    st = R.start.tolist()
    recs, pairs = [], {}
    for p, (name, t, a, b) in enumerate(PRUNING_PAIRS):
        pairs[name] = (idx[2 * p], idx[2 * p + 1])
        for w, spec in zip(pairs[name], (a, b)):
            recs += _window_reads(codes, st[w], st[w + 1], *spec)
    return Case("pruning", False, R, pack_reads(recs), dict(pairs=pairs))


def _pruning_condition(c, x):
    wins = x.trace["windows"]
    out = {}
    for name, t, a, b in PRUNING_PAIRS:
        wa, wb = c.notes["pairs"][name]
        ta, tb = wins[wa], wins[wb]
        assert (ta["n_int"], ta["n_pre"], ta["n_suf"]) == a[:3] and (tb["n_int"], tb["n_pre"], tb["n_suf"]) == b[:3] and ta["type"] == tb["type"] == t, (name, ta, tb)
        differ = sum(p != q for p, q in zip(a, b))
        assert differ == 1, name
        if len(a) > 3:
            assert ta["cover_margin"] == -1 and tb["cover_margin"] == 0, (name, ta, tb)
        kept = lambda w: (x.region_valid[w], [(v["n_prefix"], v["n_suffix"]) for v in x.windows if v["region"] == w])
        assert kept(wa) != kept(wb), (name, kept(wa), kept(wb))
        out[name] = f"{kept(wa)} / {kept(wb)}"
    # which rule each pair turns on
    w = lambda name, i: wins[c.notes["pairs"][name][i]]
    assert not w("internal_2_3", 0)["valid"] and w("internal_2_3", 1)["valid"]
    assert not w("prefix_2_3", 0)["enough"] and w("prefix_2_3", 1)["enough"] and not w("suffix_2_3", 0)["enough"] and w("suffix_2_3", 1)["enough"]
    for name in ("internal_20_21", "internal_20_21_mw"):
        assert [(w(name, i)["c0"], w(name, i)["c1"], w(name, i)["c2"]) for i in (0, 1)] == [(False, False, False), (True, False, False)], name
    assert [(w("contrib_9_10", i)["contrib"], w("contrib_9_10", i)["c1"]) for i in (0, 1)] == [(9, False), (10, True)]
    # 0.4 x 11 = 4.4: four internal arms are enough only because of the floor; 0.4 x 14 = 5.6 likewise for five
    assert w("floor", 1)["contrib"] == 11 and w("floor", 1)["c1"] and not w("floor", 0)["c1"]
    assert w("floor_wm", 1)["contrib"] == 14 and w("floor_wm", 1)["c1"] and not w("floor_wm", 1)["c0"] and not w("floor_wm", 1)["c2"] and not w("floor_wm", 0)["c1"]
    for name in ("s_4_5_sws", "s_4_5_sw", "s_4_5_ws", "s_4_5_mws", "s_4_5_swm"):
        assert [(w(name, i)["c0"], w(name, i)["c1"], w(name, i)["c2"]) for i in (0, 1)] == [(False, False, False), (False, False, True)], name
    return out


def _file_order(long_mode=False):
    rng = np.random.default_rng(105 + long_mode)
    k = 13
    n_win = 42
    if long_mode:
        layout, at, idx = [(0, SR)], 40, []
        for i in range(16):
            idx.append(len(layout)); layout.append((at, LONG)); at += 300
            layout.append((at, SR)); at += 40
        total = at
    else:
        layout, total, idx = _isolated_windows(rng, [OTHER] * n_win, k, lambda r: int(r.integers(44, 58)))
    codes = rand_codes(rng, total)
    R = make_regions(codes, layout, k, long_mode)
    st = R.start.tolist()
    recs = []
    for w in idx:
        ws, we = st[w], st[w + 1]
        third = (we - ws) // 3
        for j in range(3):                                      # internal arms of three lengths: a deletion or an insertion inside the window
            ops = [("M", 20 + j + third), ("D", j + 1), ("M", we - ws - third - j - 1 + 20)] if j < 2 else [("M", 20 + j + third), ("I", 2), ("M", we - ws - third + 20)]
            recs.append(make_read(codes, ws - 20 - j, ops, rng))
        for j in range(3):
            recs.append(exact(codes, ws - 20 - 2 * j, ws + 2 * third - 3 * j - j * j))
            recs.append(exact(codes, we - 2 * third + 2 * j + j * j, we + 20 + j))
    if not long_mode:
        while len(recs) < 400:
            w = idx[int(rng.integers(0, 8))]                   # (the first windows get a tenth and an eleventh read)
            recs.append(exact(codes, st[w] - 15, st[w] + 9 + len(recs) % 7))
        assert len(recs) == 400
    order = rng.permutation(len(recs))
    recs = [recs[i] for i in order]
    return Case("long_file_order" if long_mode else "file_order", long_mode, R, pack_reads(recs, file_rank="keep"), {})


def _file_order_condition(c, x):
    rank = c.reads.file_rank
    n = rank.size
    displaced = int((np.abs(rank.astype(np.int64) - np.arange(n)) > n // 8).sum())
    assert displaced > n // 2, displaced
    good = 0
    for ind, w in x.trace["windows"].items():
        if not w["valid"]:
            continue
        groups = {INTERNAL: [], PREFIX: [], SUFFIX: []}
        for kind, a in w["kept_from"]:
            groups[kind].append(a)
        win = [v for v in x.windows if v["region"] == ind][0]
        lens = x.arm_len[win["first_arm"]:win["first_arm"] + win["n_internal"] + win["n_prefix"] + win["n_suffix"]]
        at, ok = 0, True
        for kind in (INTERNAL, PREFIX, SUFFIX):
            g = groups[kind]
            nb = [(l + 3) // 4 for l in lens[at:at + len(g)]]
            at += len(g)
            ok = ok and len(g) >= 3 and g != sorted(g) and len(set(nb)) > 1 and len(set(l % 4 for l in lens[at - len(g):at])) > 1
        good += ok
    assert good >= 5, good
    plain = ac.build(c.regions, c.reads, c.long_mode, use_file_rank=False)
    assert plain.arms2 != x.arms2 and plain.summary == x.summary and sorted(plain.arm_len) == sorted(x.arm_len)
    return dict(windows_with_every_group_out_of_order=good, records_more_than_an_eighth_of_the_file_from_their_place=displaced)


def _span_search():
    rng = np.random.default_rng(106)
    k = 13
    # OTHER windows of 8 .. 60 bases; region `target` is 8 bases long, so that a 1-base arm passes the coefficient test
    layout, at = [], 0
    for i in range(260):
        layout.append((at, SR if i % 10 == 0 else OTHER))
        at += 40 if i % 10 == 0 else 8 if i == 233 else int(rng.integers(20, 60))
    total = at
    codes = rand_codes(rng, total)
    R = make_regions(codes, layout, k)
    st = R.start.tolist()
    span = 5003
    ws = st[233]
    recs = [exact(codes, ws - span + 1, ws + 1),                 # ends one base into the window: the furthest start that can reach it
            exact(codes, ws - span, ws),                         # one base earlier: ends on the border
            exact(codes, 17, 17 + span), exact(codes, st[120] - 1000, st[120] - 1000 + span)]
    for j in range(4):                                          # four internal arms and no other read of ordinary length: the prefix arm stays
        recs.append(exact(codes, ws - 40 - j, ws + 8 + 40 + j))
    while len(recs) < 608:
        ln = int(rng.integers(90, 111))
        rb = int(rng.integers(0, total - ln))
        if rb + ln < ws - 2 or rb > ws + 10:
            recs.append(exact(codes, rb, rb + ln))
    return Case("span_search", False, R, pack_reads(recs), dict(target=233, span=span))


def _span_search_condition(c, x):
    A, w, span = c.reads, c.notes["target"], c.notes["span"]
    ws = int(c.regions.start[w])
    spans = (A.re.astype(np.int64) - A.rb)
    assert spans.max() == span and int((spans == span).sum()) == 4 and A.rb.size == 608
    near = [a for a in range(A.rb.size) if int(A.rb[a]) == ws - span + 1 and spans[a] == span]
    far = [a for a in range(A.rb.size) if int(A.rb[a]) == ws - span and spans[a] == span]
    assert len(near) == 1 and len(far) == 1
    from_near = [r for r in x.trace["arms"] if r["a"] == near[0] and r["windex"] == w]
    assert len(from_near) == 1 and from_near[0]["result"] == "kept" and from_near[0]["kind"] == PREFIX
    assert not [r for r in x.trace["arms"] if r["a"] == far[0] and r["windex"] == w]
    assert x.region_valid[w] == 1 and (PREFIX, near[0]) in x.trace["windows"][w]["kept_from"]
    return dict(max_span=span, window=w)


def _packing():
    rng = np.random.default_rng(107)
    layout, at = [], 0
    for i in range(90):
        layout.append((at, OTHER))
        at += int(rng.integers(21, 47))
    codes = rand_codes(rng, at)
    R = make_regions(codes, layout, 13)
    recs = []
    for n in range(420):
        ln = int(rng.integers(60, 140))
        rb = int(rng.integers(0, at - ln))
        recs.append(exact(codes, rb, rb + ln))
    return Case("packing", False, R, pack_reads(recs, odd_offsets=True), {})


def _packing_condition(c, x):
    st = c.regions.start.tolist()
    wins = Counter((st[v["region"]] % 2, v["draft_len"] % 2) for v in x.windows)
    arms = Counter()
    for r in x.trace["arms"]:
        if r["result"] == "kept":
            arms[r["qb"] % 4, (r["qe"] - r["qb"]) % 4] += 1
    assert len(wins) == 4 and len(arms) == 16 and min(arms.values()) >= 3, (wins, arms)
    assert (c.reads.seq_off % 2 == 1).all()
    return dict(windows={str(k): v for k, v in sorted(wins.items())}, fewest_arms_of_a_combination=min(arms.values()))


def _two_contigs():
    """two contigs as one coordinate space (include/hypo_gpu.h): the first has an odd length, so a 1-base filler region of type SR (rank 0)
    follows and the second starts on an even position; its SRs carry on the ranks of the first"""
    rng = np.random.default_rng(108)
    k = 13
    layout, at = [], 0
    for ctg in range(2):
        for t in [SR, SW, OTHER, WS] * 9 + [SR, SW, OTHER]:
            layout.append((at, t))
            at += 40 if t == SR else int(rng.integers(24, 50))
        if ctg == 0:
            if at % 2 == 0:
                at += 1                                        # (the last window of the first contig one base longer: an odd length)
            la = at
            layout.append((la, SR))                            # the filler
            at += 1
    total = at
    codes = rand_codes(rng, total)
    R = make_regions(codes, layout, k)
    recs = []
    for n in range(40):
        ln = int(rng.integers(60, 160))
        recs.append(exact(codes, la - ln, la) if n % 2 else exact(codes, la + 1, la + 1 + ln))
    for n in range(260):
        ln = int(rng.integers(60, 160))
        lo, hi = (0, la - ln) if n % 2 else (la + 1, total - ln)
        rb = int(rng.integers(lo, hi))
        recs.append(exact(codes, rb, rb + ln))
    return Case("two_contigs", False, R, pack_reads(recs), dict(la=la))


def _two_contigs_condition(c, x):
    la = c.notes["la"]
    R, A = c.regions, c.reads
    i = R.start.tolist().index(la)
    assert la % 2 == 1 and int(R.type[i]) == SR and int(R.start[i + 1]) == la + 1 and int(R.info[i]) == 0
    ends, begins = int((A.re == la).sum()), int((A.rb == la + 1).sum())
    assert ends >= 10 and begins >= 10 and not ((A.rb <= la) & (A.re > la)).any()
    before, behind = sum(x.region_valid[:i]), sum(x.region_valid[i + 1:])
    assert before >= 5 and behind >= 5
    return dict(reads_ending_on_the_last_base=ends, reads_beginning_on_the_first_base=begins)


def _blocks():
    rng = np.random.default_rng(109)
    layout, at = [], 0
    for i in range(1130):
        layout.append((at, SR if i % 50 == 49 else OTHER))
        at += 30 if i % 50 == 49 else int(rng.integers(4, 9))
    codes = rand_codes(rng, at)
    R = make_regions(codes, layout, 13)
    recs = []
    for n in range(1301):
        ln = int(rng.integers(60, 90))
        rb = int(rng.integers(0, at - ln))
        recs.append(exact(codes, rb, rb + ln))
    return Case("blocks", False, R, pack_reads(recs), {})


def _blocks_condition(c, x):
    R, A = c.regions, c.reads
    assert R.n_regions > 1024 and R.n_regions % 256 and A.rb.size > 1024 and A.rb.size % 256
    touch = [int(np.searchsorted(R.start, int(e), "left")) - (int(np.searchsorted(R.start, int(b), "right")) - 1) for b, e in zip(A.rb, A.re)]
    assert min(touch) >= 2 and sum(touch[:1024]) > 1024 and sum(touch[1024:]) > 0        # the second block of the scan starts from a carry
    valid = x.region_valid
    assert sum(valid[:1024]) > 256 and sum(valid[1024:]) > 20                               # ... and so do the scans over the regions
    return dict(regions=R.n_regions, alignments=int(A.rb.size), touched=sum(touch), windows=sum(valid))


MANY = 1_048_576


def _many_regions():
    rng = np.random.default_rng(110)
    n = MANY + 2048 + 77
    lens = rng.integers(1, 4, size=n).astype(np.int64)
    start = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    total = int(start[n])
    codes = rand_codes(rng, total)
    rtype = np.full(n + 1, OTHER, dtype=np.uint8)
    info = np.zeros(n + 1, dtype=np.uint32)
    anchors = np.zeros(1, dtype=np.uint64)
    R = Regions(n, start, rtype, info, 1, anchors, 13, pack4(codes), codes)
    recs = []
    for centre in (MANY - 40, MANY + 40):
        c0 = int(start[centre])
        for j in range(12):
            recs.append(exact(codes, c0 - 30 - j, c0 + 30 + 2 * j))
    return Case("many_regions", False, R, pack_reads(recs), {})


def _many_regions_condition(c, x):
    assert c.regions.n_regions > MANY + 2048
    before, behind = sum(x.region_valid[:MANY]), sum(x.region_valid[MANY:])
    assert before >= 3 and behind >= 3 and x.region_valid[MANY - 40] and x.region_valid[MANY + 40]
    return dict(regions=c.regions.n_regions, windows_in_front=before, windows_behind=behind)


# ---- long mode ---------------------------------------------------------------------------------------------------------------------

def noisy_read(codes, rb, re, rng, err):
    """a read over [rb, re) with substitutions, insertions and deletions at rate err; the CIGAR says where they are"""
    ops, run, pos = [], 0, rb
    def flush():
        nonlocal run
        if run:
            ops.append(("M", run)); run = 0
    while pos < re:
        r = rng.random()
        if r < err / 3 and pos + 1 < re and run:
            flush(); ops.append(("X", 1)); pos += 1
        elif r < 2 * err / 3 and run:
            flush(); ops.append(("I", int(rng.integers(1, 3))))
        elif r < err and pos + 3 < re and run:
            flush(); d = int(rng.integers(1, 3)); ops.append(("D", d)); pos += d
        else:
            run += 1; pos += 1
    flush()
    # (pos may have run past re by a deletion: the span is what the CIGAR says)
    return make_read(codes, rb, ops, rng)


def long_layout(n, rng, win_len, sr_len=lambda r: int(r.integers(5, 60)), first_sr=True):
    layout, at = [], 0
    for i in range(n):
        if first_sr or i:
            layout.append((at, SR)); at += sr_len(rng)
        layout.append((at, LONG)); at += win_len(rng)
        if i % 3 == 1:                                          # two LONG windows side by side
            layout.append((at, LONG)); at += win_len(rng)
    layout.append((at, SR)); at += 30
    return layout, at


def _long_geometry():
    rng = np.random.default_rng(201)
    layout, total = long_layout(9, rng, lambda r: int(r.integers(300, 900)))
    codes = rand_codes(rng, total)
    R = make_regions(codes, layout, 10, True)
    st = R.start.tolist()
    recs = []
    for n in range(70):
        ln = int(rng.integers(500, 3000))
        rb = int(rng.integers(0, total - ln))
        re = rb + ln
        if n % 4 == 0:                                          # begins / ends on a border: the first / last arm is internal
            rb = st[int(np.searchsorted(R.start, rb))]
        if n % 4 == 1:
            re = st[int(np.searchsorted(R.start, re))]
        if re - rb < 200:
            continue
        recs.append(noisy_read(codes, rb, min(re, total), rng, 0.05 + 0.05 * rng.random()))
    for n in range(30):                                         # garbage over a LONG window: the filter refuses it
        w = [i for i, (_, t) in enumerate(layout) if t == LONG][n % 12]
        ws, we = st[w], st[w + 1]
        ln = we - ws + 80
        if ws < 40 or ws - 40 + ln > total:
            continue
        recs.append((ws - 40, ws - 40 + ln, rng.integers(0, 4, size=ln).tolist(), [(ln << 4) | 0]))
    lw = [i for i, (_, t) in enumerate(layout) if t == LONG and i + 1 < len(layout) and layout[i + 1][1] == LONG]
    for n, w in enumerate(lw[:3] * 2):
        ws, mid, we = st[w], st[w + 1], st[w + 2]
        # a first arm of no bases: the read begins with a deletion up to the border (S in front); a last arm of none likewise
        recs.append(make_read(codes, mid - 7, [("S", 4), ("D", 7), ("M", 300)], rng))
        recs.append(make_read(codes, mid - 300, [("M", 300), ("D", 9)], rng))
        # equal break points in the middle: a deletion over the whole second window and beyond
        if w + 3 < len(st):
            recs.append(make_read(codes, mid - 250, [("M", 250), ("D", we - mid + 3), ("M", 40)], rng))
    srs = [i for i, (_, t) in enumerate(layout) if t == SR and st[i + 1] - st[i] >= 20]
    for w in srs[:6]:                                           # over an SR only
        recs.append(exact(codes, st[w] + 2, st[w + 1] - 2))
    return Case("long_geometry", True, R, pack_reads(recs), {})


def _long_geometry_condition(c, x):
    la = x.trace["long_arms"]
    zero_first = sum(1 for r in la if r["len"] == 0 and r["kind"] == SUFFIX)
    zero_last = sum(1 for r in la if r["len"] == 0 and r["kind"] == PREFIX)
    empties = sum(w["n_empty"] for w in x.trace["windows"].values())
    kept, refused = sum(r["kept"] for r in la), sum(not r["kept"] for r in la)
    assert zero_first >= 1 and zero_last >= 1 and empties >= 1 and x.trace["single_region"] >= 3, (zero_first, zero_last, empties, x.trace["single_region"])
    assert kept >= 10 and refused >= 10
    types = set(int(t) for t in c.regions.type[:c.regions.n_regions])
    assert types == {SR, LONG}
    return dict(arms_kept=kept, arms_refused=refused, first_arms_of_no_bases=zero_first, last_arms_of_no_bases=zero_last, empty_arms=empties, reads_inside_one_region=x.trace["single_region"])


def _long_filter_edges():
    """Arms whose hits x 50 - length is 0 and -1: a copy of the draft keeps every minimizer, so its hits are known; random bases
    behind the copy lengthen the arm without a hit until the margin is the one wanted."""
    rng = np.random.default_rng(202)
    layout, total = long_layout(8, rng, lambda r: int(r.integers(400, 700)), sr_len=lambda r: 260)
    codes = rand_codes(rng, total)
    R = make_regions(codes, layout, 10, True)
    st = R.start.tolist()
    recs = []
    lw = [i for i, (_, t) in enumerate(layout) if t == LONG and layout[i - 1][1] == SR]
    made = Counter()
    for w in lw:
        ws, we = st[w], st[w + 1]
        dmin = ac.draft_minimizers(R.contig4, ws, we)
        for copy in (30, 40, 50, 60, 75, 90):
            for want in (0, -1):
                # a prefix arm: the read ends `copy` + junk bases into the window; the junk is an insertion in front of its last base
                head = codes[ws:ws + copy].tolist()
                junk_len = 20
                for _ in range(40):
                    if junk_len < 1 or junk_len > 250:
                        break
                    junk = rng.integers(0, 4, size=junk_len).tolist()
                    arm = head[:-1] + junk + head[-1:]
                    r2 = {}
                    ac.arm_is_good(arm, dmin, r2)
                    junk_len += r2["margin"] - want
                    if r2["margin"] == want:
                        lead = 200
                        q = codes[ws - lead:ws].tolist() + arm
                        recs.append((ws - lead, ws + copy, q, [((lead + copy - 1) << 4) | 0, (junk_len << 4) | 1, (1 << 4) | 0]))
                        made[want] += 1
                        break
        for ln in (3, 9, 12, 18):                               # arms shorter than 19 bases: no window of ten 10-mers, no hit
            recs.append(exact(codes, ws - 250, ws + ln))
            recs.append(exact(codes, we - ln, min(we + 240, total)))
        recs.append(make_read(codes, ws - 200, [("M", 200), ("D", 9)], rng))                   # a last arm of no bases
    return Case("long_filter_edges", True, R, pack_reads(recs), {})


def _long_filter_edges_condition(c, x):
    la = x.trace["long_arms"]
    zero, minus, short, empty = (sum(1 for r in la if r["len"] > 0 and r["margin"] == 0), sum(1 for r in la if r["margin"] == -1),
                                 sum(1 for r in la if 0 < r["len"] < 19), sum(1 for r in la if r["len"] == 0))
    assert zero >= 5 and minus >= 5 and short >= 5 and empty >= 5, (zero, minus, short, empty)
    assert all(r["kept"] == (r["margin"] >= 0) for r in la) and all(r["hits"] == 0 and not r["kept"] for r in la if 0 < r["len"] < 19)
    return dict(margin_0=zero, margin_minus_1=minus, shorter_than_19=short, no_bases=empty)


def _long_ties():
    rng = np.random.default_rng(203)
    layout, total = long_layout(6, rng, lambda r: int(r.integers(400, 700)))
    codes = rand_codes(rng, total)
    at = 50
    while at + 40 < total:                                      # homopolymers and period-2 stretches of 14 .. 30 bases every 60 or so
        ln = int(rng.integers(14, 31))
        b = int(rng.integers(0, 4))
        codes[at:at + ln] = b if rng.integers(0, 2) else np.resize([b, (b + 1 + int(rng.integers(0, 3))) % 4], ln)
        at += ln + int(rng.integers(30, 60))
    # eleven A, then (AC) x 10, then bases whose k-mers all have larger keys: the key of ACACACACAC stands at every other position, smaller
    # keys stand in front of the first and none follows within a window.  The queue shows every one of them as the earliest in turn; a
    # scan that took the latest of equal keys would never show the first few (a window that ends on one of them still holds a smaller key)
    st = [s for s, _ in layout] + [total]
    lw = [i for i, (_, t) in enumerate(layout) if t == LONG and st[i] >= 30][:6]
    for w in lw:
        ws = st[w]
        codes[ws + 20:ws + 51] = [0] * 11 + [0, 1] * 10
        for _ in range(400):
            codes[ws + 51:ws + 65] = rng.integers(0, 4, size=14)
            dmin = ac.draft_minimizers(pack4(codes), ws, st[w + 1])
            head = codes[ws:ws + 75].tolist()
            if ac.arm_hits(head, dmin)[1] >= ac.arm_hits(head, dmin, latest_of_equal=True)[1] + 3:
                break
    R = make_regions(codes, layout, 10, True)
    recs = []
    for n in range(40):
        ln = int(rng.integers(500, 1500))
        rb = int(rng.integers(0, total - ln))
        recs.append(noisy_read(codes, rb, rb + ln, rng, 0.03))
    # prefix arms that are a copy of the window's first bases with random bases in front of the last one, as many as it takes for
    # hits x 50 - length to be 0: one hit less and the arm would go
    for w in lw:
        ws = st[w]
        dmin = ac.draft_minimizers(R.contig4, ws, st[w + 1])
        for copy in (75, 90):
            head, junk_len = codes[ws:ws + copy].tolist(), 20
            for _ in range(40):
                if junk_len < 1 or junk_len > 2500:
                    break
                arm = head[:-1] + rng.integers(0, 4, size=junk_len).tolist() + head[-1:]
                r2 = {}
                ac.arm_is_good(arm, dmin, r2)
                if r2["margin"] == 0:
                    recs.append((ws - 30, ws + copy, codes[ws - 30:ws].tolist() + arm, [((30 + copy - 1) << 4) | 0, (junk_len << 4) | 1, (1 << 4) | 0]))
                    break
                junk_len += r2["margin"]
    return Case("long_ties", True, R, pack_reads(recs), {})


def _long_ties_condition(c, x):
    R = c.regions
    draft_ties = []
    for i in range(R.n_regions):
        if int(R.type[i]) == LONG:
            ac.minimizer_windows([ac.contig_code(R.contig4, p) for p in range(int(R.start[i]), int(R.start[i + 1]))], ties=draft_ties)
    assert len(x.trace["ties"]) >= 100 and len(draft_ties) >= 100, (len(x.trace["ties"]), len(draft_ties))
    kept = sum(r["kept"] for r in x.trace["long_arms"])
    assert kept >= 10
    # arms the filter keeps with nothing to spare that the latest of equal keys would have lost
    turn = sum(1 for r in x.trace["long_arms"] if r["margin"] == 0 and r["len"] > 0 and r["margin_if_latest_of_equal"] < 0)
    assert turn >= 5, turn
    return dict(windows_with_the_smallest_key_twice_in_arms=len(x.trace["ties"]), in_drafts=len(draft_ties), arms_kept=kept, arms_that_turn_on_which_of_equal_keys=turn)


def _long_draft_n():
    rng = np.random.default_rng(204)
    layout, total = long_layout(8, rng, lambda r: int(r.integers(300, 500)))
    codes = rand_codes(rng, total)
    st = [s for s, _ in layout] + [total]
    lw = [i for i, (_, t) in enumerate(layout) if t == LONG]
    n_runs = {}
    for j, w in enumerate(lw):
        ln = (1, 9, 10, 30)[j % 4]
        at = st[w] + 40 + 7 * j
        codes[at:at + ln] = 4
        n_runs[w] = (at, ln)
        if j % 4 == 0:
            codes[at + 23] = 4; codes[st[w] + 3] = 4            # a second N within ten k-mers of the first, and one before the first k-mer
    R = make_regions(codes, layout, 10, True)
    recs = []
    for n in range(60):
        ln = int(rng.integers(500, 1200))
        rb = int(rng.integers(0, total - ln))
        q = [b if b < 4 else int(rng.integers(0, 4)) for b in codes[rb:rb + ln].tolist()]
        recs.append((rb, rb + ln, q, [(ln << 4) | 0]))
    return Case("long_draft_n", True, R, pack_reads(recs), dict(n_runs=n_runs))


def _long_draft_n_condition(c, x):
    R = c.regions
    differ_a = differ_reset = 0
    with_a = pack4(np.where(R.codes < 4, R.codes, 0).astype(np.uint8))
    for w, (at, ln) in c.notes["n_runs"].items():
        ws, we = int(R.start[w]), int(R.start[w + 1])
        assert ws < at and at + ln < we and (R.codes[at:at + ln] == 4).all()
        real = ac.draft_minimizers(R.contig4, ws, we)
        differ_a += real != ac.draft_minimizers(with_a, ws, we)
        differ_reset += real != ac.draft_minimizers(R.contig4, ws, we, reset_processed_at_n=True)
    lens = sorted(set(ln for _, ln in c.notes["n_runs"].values()))
    assert lens == [1, 9, 10, 30] and differ_a == len(c.notes["n_runs"]) and differ_reset >= 4, (lens, differ_a, differ_reset)
    kept = sum(r["kept"] for r in x.trace["long_arms"])
    assert kept >= 10
    return dict(drafts_with_n=differ_a, drafts_where_a_reset_of_processed_would_show=differ_reset, arms_kept=kept)


LONG_PRUNING = [("internal_10_11", (10, 0), (11, 0)), ("with_empties_10_11", (7, 3), (7, 4)), ("all_empty_10_11", (1, 9), (1, 10))]


def _long_pruning():
    rng = np.random.default_rng(205)
    layout, at, idx = [(0, SR)], 300, []
    for i in range(2 * len(LONG_PRUNING)):
        idx.append(len(layout)); layout.append((at, LONG)); at += 260
        layout.append((at, SR)); at += 300
    codes = rand_codes(rng, at)
    R = make_regions(codes, layout, 10, True)
    st = R.start.tolist()
    recs, pairs = [], {}
    for p, (name, a, b) in enumerate(LONG_PRUNING):
        pairs[name] = (idx[2 * p], idx[2 * p + 1])
        for w, (n_int, n_empty) in zip(pairs[name], (a, b)):
            ws, we = st[w], st[w + 1]
            for j in range(n_int):
                recs.append(exact(codes, ws - 150 - j, we + 150 + j))
            for j in range(n_empty):
                recs.append(make_read(codes, ws - 200 - j, [("M", 198 + j), ("D", we - ws + 5), ("M", 200)], rng))
            for j in range(2):
                recs.append(exact(codes, ws - 200 - j, ws + 150 + 7 * j))
                recs.append(exact(codes, we - 140 - 5 * j, we + 220 + j))
    return Case("long_pruning", True, R, pack_reads(recs), dict(pairs=pairs))


def _long_pruning_condition(c, x):
    out = {}
    for name, a, b in LONG_PRUNING:
        wa, wb = c.notes["pairs"][name]
        ta, tb = x.trace["windows"][wa], x.trace["windows"][wb]
        assert (ta["n_int"], ta["n_empty"], ta["n_pre"], ta["n_suf"]) == a + (2, 2) and (tb["n_int"], tb["n_empty"], tb["n_pre"], tb["n_suf"]) == b + (2, 2), (name, ta, tb)
        assert ta["internal"] == 10 and tb["internal"] == 11 and not ta["clear"] and tb["clear"]
        va, vb = ([v for v in x.windows if v["region"] == w][0] for w in (wa, wb))
        assert (va["n_prefix"], va["n_suffix"], vb["n_prefix"], vb["n_suffix"]) == (2, 2, 0, 0)
        out[name] = "prefix and suffix arms kept / dropped"
    return out


BUILDERS = dict(corners=_corners, empty_arms=_empty_arms, anchors_k5=lambda: _anchors(5, 1035), anchors_k13=lambda: _anchors(13, 1033), anchors_k31=lambda: _anchors(31, 1031),
                pruning=_pruning, file_order=_file_order, span_search=_span_search, packing=_packing, two_contigs=_two_contigs, blocks=_blocks,
                many_regions=_many_regions, long_geometry=_long_geometry, long_filter_edges=_long_filter_edges, long_ties=_long_ties,
                long_draft_n=_long_draft_n, long_pruning=_long_pruning, long_file_order=lambda: _file_order(True))
CONDITIONS = dict(corners=_corners_condition, empty_arms=_empty_arms_condition, anchors_k5=_anchors_condition, anchors_k13=_anchors_condition,
                  anchors_k31=_anchors_condition, pruning=_pruning_condition, file_order=_file_order_condition, span_search=_span_search_condition,
                  packing=_packing_condition, two_contigs=_two_contigs_condition, blocks=_blocks_condition, many_regions=_many_regions_condition,
                  long_geometry=_long_geometry_condition, long_filter_edges=_long_filter_edges_condition, long_ties=_long_ties_condition,
                  long_draft_n=_long_draft_n_condition, long_pruning=_long_pruning_condition, long_file_order=_file_order_condition)
SHORT_CASES = [n for n in BUILDERS if not n.startswith("long_")]
LONG_CASES = [n for n in BUILDERS if n.startswith("long_")]
CASES = SHORT_CASES + LONG_CASES


@functools.lru_cache(maxsize=None)
def case(name):
    c = BUILDERS[name]()
    assert c.name == name
    check_tables(c)
    return c


@functools.lru_cache(maxsize=None)
def expected(name):
    """what tests/arms_checker.py says the device must return for the case (shared by the tests; nobody changes it)"""
    c = case(name)
    return ac.build(c.regions, c.reads, c.long_mode)


@functools.lru_cache(maxsize=None)
def condition(name):
    """asserts what the case is there for; returns the counts it reached (tests/README_arms.md lists them)"""
    return CONDITIONS[name](case(name), expected(name))


WINDOW_DTYPE = np.dtype([("type", "u1"), ("reserved", "u1", 3), ("draft_len", "<u4"), ("draft_off", "<u8"), ("first_arm", "<u4"), ("n_internal", "<u4"),
                         ("n_prefix", "<u4"), ("n_suffix", "<u4"), ("n_empty", "<u4"), ("reserved2", "<u4")])      # HypoWindow, 40 bytes


def as_arrays(x):
    """the checker's result as the arrays hypo_gpu_arms_download fills (reserved fields 0)"""
    win = np.zeros(len(x.windows), dtype=WINDOW_DTYPE)
    for i, v in enumerate(x.windows):
        for f in ("type", "draft_len", "draft_off", "first_arm", "n_internal", "n_prefix", "n_suffix", "n_empty"):
            win[f][i] = v[f]
    return dict(windows=win, win_region=np.array(x.win_region, dtype=np.uint32), arm_len=np.array(x.arm_len, dtype=np.uint32),
                arm_off=np.array(x.arm_off, dtype=np.uint64), arms2=np.frombuffer(x.arms2, dtype=np.uint8), draft4=np.frombuffer(x.draft4, dtype=np.uint8))
