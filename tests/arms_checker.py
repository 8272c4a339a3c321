"""Arm selection restated in plain Python: what hypo_gpu_arms_build / _build_long followed by hypo_gpu_arms_download / _download_long
must return for the flat arrays of HypoArmsRegions and HypoArmsReads (include/hypo_gpu.h).  Written from the host loops —
Alignment::find_short_arms, find_long_arms, find_bp, prepare_short_arm and add_arms (host/Alignment.cpp), Contig::fill_short_windows
and fill_long_windows (host/Contig.cpp), Window::add_* and Filter (host/Window.hpp, host/Filter.hpp), PackedSeq::check_kmer and
find_kmer — one alignment after the other, lists and loops, no device layout.  tests/test_arms_checker_cpu.py pins it to those
loops on every case of tests/arms_cases.py; tests/test_gpu_arms_direct.py pins the kernels of arms_kernel.hip to it.

build() also fills a trace: how every break point was decided, what every anchor search did, the minimizers and hits of every long
arm, the counts of every window before pruning.  The cases assert from it that they reach what they are there for."""
from bisect import bisect_left, bisect_right
from collections import Counter

SWS, SW, WS, MWM, MW, WM, SWM, MWS, OTHER, LONG, SR, MSR = range(12)        # RegionType (host/Settings.hpp)
TYPE_NAMES = ["SWS", "SW", "WS", "MWM", "MW", "WM", "SWM", "MWS", "OTHER", "LONG", "SR", "MSR"]
INTERNAL, PREFIX, SUFFIX, EMPTY = "I", "P", "S", "E"
# ArmsSettings / MinimizerSettings (host/Settings.hpp)
MIN_SHORT_NUM, MIN_INTERNAL1, MIN_INTERNAL2, MIN_INTERNAL3, MIN_CONTRIB, MIN_INTERNAL_CONTRIB, SHORT_ARM_COEF, MK = 3, 20, 5, 10, 10, 0.4, 10, 10
FILTER_K, FILTER_W, BP_PER_MINIMIZER = 10, 10, 50                           # host/Filter.hpp
CIGAR_TYPE = {0: 3, 1: 1, 2: 2, 3: 2, 4: 1, 5: 0, 6: 0, 7: 3, 8: 3}        # bit 0 consumes the query, bit 1 the reference


def is_sr(t):
    return t == SR or t == MSR


def read_codes(reads2, seq_off, qae):
    """the qae bases of the PackedSeq<2> that starts at byte seq_off"""
    out = []
    for i in range(qae):
        out.append((int(reads2[seq_off + (i >> 2)]) >> (6 - 2 * (i & 3))) & 3)
    return out


def contig_code(contig4, p):
    return (int(contig4[p >> 1]) >> (4 - 4 * (p & 1))) & 15


def kmer_of(codes, at, k):
    v = 0
    for i in range(k):
        v = (v << 2) | codes[at + i]
    return v


def find_kmer(rd, target, k, left, right, first):
    """PackedSeq::find_kmer: (first or last start of target among the k-mers inside [left, right) or None, number of such starts)"""
    hit, n = None, 0
    for s in range(left, right - k + 1):
        if kmer_of(rd, s, k) == target:
            n += 1
            if hit is None or not first:
                hit = s
    return hit, n


def find_bp(starts, types, rb, cigar, beg, end, how):
    """Alignment::find_bp: the query positions where the read crosses the borders of regions beg .. end - 1"""
    res = []
    ref_pos, cur, qpos, corner = rb, beg + 1, 0, False
    next_ref = starts[cur]
    for c in cigar:
        op, ln = c & 15, c >> 4
        if op == 4 or op == 5:
            continue
        t = CIGAR_TYPE[op]
        if t & 2:
            both = t == 3
            if corner:
                res.append(qpos); how.append("corner_M" if both else "corner_DN")
                corner = False; cur += 1; next_ref = starts[cur]
            while ref_pos + ln >= next_ref and not corner:
                d = next_ref - ref_pos
                ref_pos = next_ref
                if both:
                    qpos += d
                ln -= d
                if ln > 0:
                    res.append(qpos); how.append("inside")
                    cur += 1; next_ref = starts[cur]
                else:
                    corner = True
            if ln > 0:
                ref_pos += ln
                if both:
                    qpos += ln
        elif t & 1:
            if corner:
                left_sr = is_sr(types[cur - 1])
                res.append(qpos if left_sr else qpos + ln); how.append("corner_I_sr" if left_sr else "corner_I_win")
                cur += 1; next_ref = starts[cur]; corner = False
            qpos += ln
        if cur == end:
            break
    return res


def prepare_short_arm(R, rd, qae, windex, qb, qe, kind, rec):
    """Alignment::prepare_short_arm: (q_beg, q_end) of the arm of window windex, or None; rec takes what happened"""
    k = R.k
    curr, nxt = R.starts[windex], R.starts[windex + 1]
    rec["coef_margin"] = SHORT_ARM_COEF * (qe - qb) - (nxt - curr)
    if nxt - curr > SHORT_ARM_COEF * (qe - qb):
        rec["result"] = "coef"
        return None
    wt = R.types[windex]
    valid, q_beg, q_end = True, qb, qe

    def side(name, anchor, kk, far, near):
        """one of the four searches; far / near: how many bases the range reaches outwards / into the arm"""
        nonlocal valid, q_beg, q_end
        s = dict(outcome=None, moved=0, hits=0, clamp0=False, clampq=False)
        rec[name] = s
        if name[0] == "L":
            if q_beg < kk:
                valid = False; s["outcome"] = "edge"
                return
            if kmer_of(rd, q_beg - kk, kk) == anchor:
                s["outcome"] = "exact"
                return
            lo = 0 if q_beg < far else q_beg - far
            hi = q_end if q_end < q_beg + near else q_beg + near
            s["clamp0"] = q_beg < far
            hit, s["hits"] = find_kmer(rd, anchor, kk, lo, hi, False)
            if hit is None:
                valid = False; s["outcome"] = "notfound"
            else:
                s["outcome"], s["moved"] = "moved", hit + kk - q_beg
                q_beg = hit + kk
        else:
            if q_end + kk > qae:
                valid = False; s["outcome"] = "edge"
                return
            if kmer_of(rd, q_end, kk) == anchor:
                s["outcome"] = "exact"
                return
            lo = q_beg if q_end < q_beg + near else q_end - near
            hi = qae if qae < q_end + far else q_end + far
            s["clampq"] = qae < q_end + far
            hit, s["hits"] = find_kmer(rd, anchor, kk, lo, hi, True)
            if hit is None:
                valid = False; s["outcome"] = "notfound"
            else:
                s["outcome"], s["moved"] = "moved", hit - q_end
                q_end = hit

    if wt in (SWS, SW, SWM) and kind != SUFFIX:
        side("LS", R.anchors[R.info[windex - 1] << 1], k, 2 * k, k)
    if wt in (SWS, WS, MWS) and kind != PREFIX:
        side("RS", R.anchors[(R.info[windex + 1] << 1) - 1], k, 2 * k, k)
    if wt in (MWM, MW, MWS) and kind != SUFFIX:
        side("LM", R.info[windex - 1], MK, 3 * MK, 2 * MK)
    if wt in (MWM, WM, SWM) and kind != PREFIX:
        side("RM", R.info[windex + 1], MK, 3 * MK, 2 * MK)
    if valid and q_beg < q_end:
        rec["result"] = "kept"
        return q_beg, q_end
    rec["result"] = "crossed" if valid else "invalid"
    return None


def minimizer_windows(codes, reset_processed_at_n=False, latest_of_equal=False, ties=None):
    """Filter::scan: the (canonical k-mer, position of its last base) the monotone queue of the last W k-mers has in front, once
    per k-mer from the W-th on.  codes >= 4 are N: the run of bases starts again, the count of k-mers does not.
    (reset_processed_at_n and latest_of_equal give OTHER functions, for the conditions of cases: the count starting again at an N;
    the latest instead of the earliest of equal smallest keys.)  ties: a list that takes 1 per window whose smallest key is there twice"""
    mask, shift = (1 << (2 * FILTER_K)) - 1, 2 * (FILTER_K - 1)
    fwd = rev = run = processed = 0
    q, out = [], []
    for i, c in enumerate(codes):
        if c >= 4:
            run = 0
            if reset_processed_at_n:
                processed = 0
            continue
        run += 1
        fwd = ((fwd << 2) | c) & mask
        rev = (rev >> 2) | ((3 ^ c) << shift)
        canon = fwd if fwd < rev else rev
        if run < FILTER_K:
            continue
        while q and q[-1][0] > canon:
            q.pop()
        q.append((canon, i))
        while q[0][1] + FILTER_W <= i:
            q.pop(0)
        processed += 1
        if processed >= FILTER_W:
            front = q[0]
            if latest_of_equal:
                for e in q:
                    if e[0] == front[0]:
                        front = e
            out.append(front)
            if ties is not None and len(q) > 1 and q[1][0] == q[0][0]:
                ties.append(1)
    return out


def draft_minimizers(contig4, ws, we, **kw):
    return set(m[0] for m in minimizer_windows([contig_code(contig4, p) for p in range(ws, we)], **kw))


def arm_hits(arm, dmin, **kw):
    found = []
    for m in minimizer_windows(arm, **kw):
        if not found or found[-1][1] != m[1]:
            found.append(m)
    hits = 0
    for m in found:
        if m[0] in dmin:
            hits += 1
    return found, hits


def arm_is_good(arm, dmin, rec, ties=None):
    """Filter::is_good: one entry per minimizer position, a hit where the draft has that minimizer, one hit per 50 bases"""
    found, hits = arm_hits(arm, dmin, ties=ties)
    rec["margin_if_latest_of_equal"] = arm_hits(arm, dmin, latest_of_equal=True)[1] * BP_PER_MINIMIZER - len(arm)      # (for a case's condition)
    rec["positions"], rec["hits"], rec["margin"] = [m[1] for m in found], hits, hits * BP_PER_MINIMIZER - len(arm)
    return hits * BP_PER_MINIMIZER >= len(arm)


class Tables:
    """the flat arrays as Python lists"""

    def __init__(self, regions):
        self.n = int(regions.n_regions)
        self.starts = [int(x) for x in regions.start]
        self.types = [int(x) for x in regions.type]
        self.info = None if regions.info is None else [int(x) for x in regions.info]
        self.anchors = None if regions.anchor_kmers is None else [int(x) for x in regions.anchor_kmers]
        self.k = int(regions.k)
        self.contig4 = regions.contig4


class Result:
    pass


def pack2(codes):
    out = bytearray((len(codes) + 3) // 4)
    for i, c in enumerate(codes):
        out[i >> 2] |= c << (6 - 2 * (i & 3))
    return bytes(out)


def build(regions, reads, long_mode=False, use_file_rank=True):
    """regions: n_regions, start, type, info, anchor_kmers, k, contig4; reads: rb, re, qae, seq_off, reads2, cigar_off, cigar, file_rank
    (None or a permutation).  Returns a Result: region_valid, summary, windows (a dict per window), arm_len, arm_off, arms2, draft4,
    arms (per window: the kept arms as (kind, codes)), trace."""
    R = Tables(regions)
    n_al = len(reads.rb)
    trace = dict(bp=Counter(), first=Counter(), last=Counter(), single_region=0, arms=[], long_arms=[], windows={}, ties=[])
    per_alignment = []                                        # the arms of every alignment: (windex, kind, codes)
    dmin = {}
    for a in range(n_al):
        rb, re, qae = int(reads.rb[a]), int(reads.re[a]), int(reads.qae[a])
        arms = []
        per_alignment.append(arms)
        beg = bisect_right(R.starts, rb) - 1                  # rank(rb), one less where rb is no border
        end = bisect_left(R.starts, re)                       # rank(re)
        if end - beg <= 1:
            trace["single_region"] += 1
            continue
        cigar = [int(c) for c in reads.cigar[int(reads.cigar_off[a]):int(reads.cigar_off[a + 1])]]
        rd = read_codes(reads.reads2, int(reads.seq_off[a]), qae)
        how = []
        bp = find_bp(R.starts, R.types, rb, cigar, beg, end, how)
        assert len(bp) == end - beg - 1, (a, bp)
        trace["bp"].update(how)
        first_kind = INTERNAL if R.starts[beg] == rb else SUFFIX
        last_kind = INTERNAL if R.starts[end] == re else PREFIX
        trace["first"][first_kind] += 1; trace["last"][last_kind] += 1
        pieces = [(beg, 0, bp[0], first_kind)]
        for i in range(1, end - beg - 1):
            pieces.append((beg + i, bp[i - 1], bp[i], INTERNAL))
        pieces.append((end - 1, bp[-1], qae, last_kind))
        for n, (ind, qb, qe, kind) in enumerate(pieces):
            middle = 0 < n < len(pieces) - 1
            if long_mode:
                if R.types[ind] != LONG:                      # (find_long_arms asks for SR; the pseudo regions are SR or LONG)
                    continue
                if middle and qb == qe:
                    arms.append((ind, EMPTY, None))
                    continue
                if ind not in dmin:
                    dmin[ind] = draft_minimizers(R.contig4, R.starts[ind], R.starts[ind + 1])
                rec = dict(a=a, windex=ind, kind=kind, len=qe - qb)
                rec["kept"] = arm_is_good(rd[qb:qe], dmin[ind], rec, trace["ties"])      # Window::add_* of a LONG window
                trace["long_arms"].append(rec)
                if rec["kept"]:
                    arms.append((ind, kind, rd[qb:qe]))
                continue
            if is_sr(R.types[ind]):
                continue
            if middle and qb == qe:
                arms.append((ind, EMPTY, None))
                continue
            rec = dict(a=a, windex=ind, wtype=R.types[ind], kind=kind, qb=qb, qe=qe, qae=qae)
            trace["arms"].append(rec)
            got = prepare_short_arm(R, rd, qae, ind, qb, qe, kind, rec)
            if got:
                arms.append((ind, kind, rd[got[0]:got[1]]))
    # Alignment::add_arms, one alignment after the other in FILE order
    order = list(range(n_al))
    if use_file_rank and getattr(reads, "file_rank", None) is not None:
        order = [0] * n_al
        for a in range(n_al):
            order[int(reads.file_rank[a])] = a
    wins = {}
    for a in order:
        for ind, kind, codes in per_alignment[a]:
            w = wins.setdefault(ind, {INTERNAL: [], PREFIX: [], SUFFIX: [], EMPTY: 0, "from": []})
            if kind == EMPTY:
                w[EMPTY] += 1
            else:
                w[kind].append(codes); w["from"].append((kind, a))
    # Contig::fill_short_windows / fill_long_windows
    kept = {}
    touched = sorted(wins) if not long_mode else [i for i in range(R.n) if R.types[i] == LONG]
    for ind in touched:
        w = wins.get(ind, {INTERNAL: [], PREFIX: [], SUFFIX: [], EMPTY: 0, "from": []})
        n_int, n_pre, n_suf, n_empty = len(w[INTERNAL]), len(w[PREFIX]), len(w[SUFFIX]), w[EMPTY]
        internal = n_int + n_empty                            # Window::get_num_internal counts the empty arms
        t = dict(type=R.types[ind], n_int=n_int, n_pre=n_pre, n_suf=n_suf, n_empty=n_empty, internal=internal)
        trace["windows"][ind] = t
        if long_mode:
            clear = internal > MIN_INTERNAL3
            t.update(valid=True, clear=clear)
        else:
            valid = True
            if internal < MIN_SHORT_NUM:
                win_len = R.starts[ind + 1] - R.starts[ind]
                max_pre = max([len(x) for x in w[PREFIX]] + [0]); max_suf = max([len(x) for x in w[SUFFIX]] + [0])
                t["covered"] = max_pre + max_suf >= win_len
                t["cover_margin"] = max_pre + max_suf - win_len
                t["enough"] = n_pre >= MIN_SHORT_NUM and n_suf >= MIN_SHORT_NUM
                valid = t["covered"] and t["enough"]
            clear = False
            if valid:
                contrib = internal + n_pre + n_suf
                t["contrib"] = contrib
                t["c0"] = internal > MIN_INTERNAL1
                t["c1"] = contrib >= MIN_CONTRIB and float(internal) >= float(int(MIN_INTERNAL_CONTRIB * float(contrib)))
                t["c2"] = R.types[ind] in (SWS, SW, WS, MWS, SWM) and internal >= MIN_INTERNAL2
                clear = t["c0"] or t["c1"] or t["c2"]
            t.update(valid=valid, clear=clear)
            if not valid:
                continue
        kept[ind] = [(INTERNAL, x) for x in w[INTERNAL]] + ([] if clear else [(PREFIX, x) for x in w[PREFIX]] + [(SUFFIX, x) for x in w[SUFFIX]])
        t["kept_from"] = [f for f in w["from"] if f[0] == INTERNAL or not clear]
    # the batch: windows in region order, the arms of a window internal, prefix, suffix, every arm and every draft on a byte boundary
    res = Result()
    res.region_valid = [0] * R.n
    res.windows, res.win_region, res.arm_len, res.arm_off, res.arms = [], [], [], [], []
    arms2, draft4 = bytearray(), bytearray()
    out_bytes = 0
    for ind in sorted(kept):
        res.region_valid[ind] = 1
        ws, we = R.starts[ind], R.starts[ind + 1]
        arms = kept[ind]
        t = trace["windows"][ind]
        res.windows.append(dict(region=ind, type=1 if long_mode else 0, draft_len=we - ws, draft_off=len(draft4), first_arm=len(res.arm_len),
                                n_internal=sum(1 for x in arms if x[0] == INTERNAL), n_prefix=sum(1 for x in arms if x[0] == PREFIX),
                                n_suffix=sum(1 for x in arms if x[0] == SUFFIX), n_empty=t["n_empty"]))
        res.win_region.append(ind)
        res.arms.append(arms)
        longest = we - ws
        for kind, codes in arms:
            res.arm_len.append(len(codes)); res.arm_off.append(len(arms2))
            arms2 += pack2(codes)
            longest = max(longest, len(codes))
        for j in range((we - ws + 1) // 2):
            hi = contig_code(R.contig4, ws + 2 * j)
            lo = contig_code(R.contig4, ws + 2 * j + 1) if 2 * j + 1 < we - ws else 0
            draft4.append((hi << 4) | lo)
        out_bytes += (longest + longest // 2 + 24 + 7) // 8 * 8          # hypo_gpu_poa_slot_layout's rule
    res.arms2, res.draft4 = bytes(arms2), bytes(draft4)
    res.summary = dict(n_windows=len(res.windows), n_arms=len(res.arm_len), arms2_bytes=len(arms2), draft4_bytes=len(draft4), out_bytes=out_bytes)
    res.trace = trace
    return res


def window_text(contig4, ws, we, arms):
    """Window::dump_text of the window over [ws, we) with these kept arms: draft|I:arm..|P:arm..|S:arm.."""
    text = "".join("ACGTN"[min(contig_code(contig4, p), 4)] for p in range(ws, we))
    for kind, codes in arms:
        text += "|" + kind + ":" + "".join("ACGT"[c] for c in codes)
    return text
