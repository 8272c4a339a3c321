"""A plain restatement of the two support votes of a mapped read, over the flat arrays the C-ABI takes (include/hypo_gpu.h:
hypo_gpu_reads_upload, hypo_gpu_support_kmers, hypo_gpu_support_minimizers).

  kmer_votes        Alignment::update_solidkmers_support in the reference's own form: a map from k-mer id to the span's solid
                    k-mers per read, every read k-mer looked up in it, equal ids visited from the highest index down.  Not the sliding
                    window of hypo_amd/csrc/host/Alignment.cpp, not the tiles and the byte screen of support_kernel.hip.
  minimizer_votes   Alignment::update_minimisers_support: the read's window minimizers collected first, then every minimizer of
                    every mega-window the read touches looked up among them.

Plain loops over Python ints; widths are applied where the reference's types apply them and nowhere else.  Meant for a few
hundred thousand read positions per call (tests/votes_cases.py keeps its cases below that)."""
import bisect
from collections import namedtuple

import numpy as np

MIN_K = 10          # Minimizer_settings: k-mer and window of the mega-window minimizers
MIN_W = 10
U16 = 0xFFFF
U32 = 0xFFFFFFFF
U64 = 0xFFFFFFFFFFFFFFFF

MegaTables = namedtuple("MegaTables", "contig_base reg_base win_even info_base start n_info mw_off rel_pos minimisers")   # HypoMegaWindows


def read_bases(reads2, off, n):
    """bases 0 .. n of the 2-bit read that starts at byte `off` (four to a byte, the first in the top bits)"""
    nb = (n + 3) // 4
    b = np.asarray(reads2[off:off + nb], dtype=np.uint8)
    return (((b[:, None] >> np.array([6, 4, 2, 0], dtype=np.uint8)) & 3).reshape(-1)[:n]).tolist()


def solid_span(spos_list, k, rb, re):
    """[first, last) of the solid k-mers a read [rb, re) covers: those that start at or behind rb, up to the last one that lies
    wholly inside the read (when none does, every one that starts in front of re stays, as in the reference)"""
    first = bisect.bisect_left(spos_list, rb)
    last = bisect.bisect_left(spos_list, re)
    for i in range(last, first, -1):
        if spos_list[i - 1] + k <= re:
            last = i
            break
    return first, last


def kmer_votes(k, spos, kids, rb, re, qae, seq_off, reads2, diag=None, id_bits=64):
    """(coverage, support) of every solid k-mer.  diag: a dict that receives the diagnostics of the case: multi = read k-mers with
    two or more candidates in the read's map, refused = votes inside [left, right] that the pvs_supp rule refused, at_left / at_right
    = votes cast with the read k-mer's offset exactly on the left / right end of [left, right].  id_bits = 32
    compares the low 32 bits of the ids only (what a narrow comparison would compute: the tests use it to show that a table tells
    the two apart)."""
    sp = [int(x) for x in spos]
    kd = [int(x) for x in kids]
    idmask = (1 << id_bits) - 1
    n = len(sp)
    cov = [0] * n
    sup = [0] * n
    multi = refused = at_left = at_right = 0
    kmask = (1 << (2 * k)) - 1
    for a in range(len(rb)):
        b, e = int(rb[a]), int(re[a])
        first, last = solid_span(sp, k, b, e)
        if last <= first:
            continue
        kmap = {}
        for i in range(first, last):
            cov[i] += 1
            kmap.setdefault(kd[i] & idmask, []).append(i - first)
        num_cbases = e - b
        pvs_kpos, pvs_rbind = -1, 0
        kmer = kmer_len = 0
        for r_ind, base in enumerate(read_bases(reads2, int(seq_off[a]), int(qae[a]))):
            kmer = ((kmer << 2) | base) & kmask
            if kmer_len < k:
                kmer_len += 1
            if kmer_len != k:
                continue
            cands = kmap.get(kmer & idmask)
            if not cands:
                continue
            if len(cands) >= 2:
                multi += 1
            r_bind = r_ind + 1 - k
            for c in reversed(cands):                       # equal ids: the one inserted last comes first
                c_dist = sp[first + c] - b
                left = c_dist - k if c_dist > k else 0
                right = min(num_cbases, c_dist + k)
                if r_bind < left or r_bind > right:
                    continue
                pos = sp[first + c]
                if pvs_kpos > -1 and pos <= k + pvs_kpos:
                    # an overlapping or adjacent neighbour voted last: the offsets in read and contig must agree (32-bit difference
                    # on the read's side, 64-bit on the contig's, as the reference's types have it)
                    if ((r_bind - pvs_rbind) & U32) != ((pos - pvs_kpos) & U64):
                        refused += 1
                        continue
                pvs_kpos, pvs_rbind = pos, r_bind
                sup[first + c] += 1
                at_left += r_bind == left
                at_right += r_bind == right
    if diag is not None:
        diag.update(multi=multi, refused=refused, at_left=at_left, at_right=at_right)
    return np.array(cov, dtype=np.uint32), np.array(sup, dtype=np.uint32)


def read_minimizers(bases):
    """[(k-mer, start)] of the read's window minimizers: forward strand, K = W = 10, the earliest of equal keys, one entry per start"""
    out = []
    mask = (1 << (2 * MIN_K)) - 1
    kmer = 0
    keys = []                                              # (k-mer, index of its last base) of every k-mer so far
    last_found = len(bases) + 1
    for i, b in enumerate(bases):
        kmer = ((kmer << 2) | b) & mask
        if i + 1 < MIN_K:
            continue
        keys.append((kmer, i))
        if len(keys) < MIN_W:
            continue
        best = min(keys[-MIN_W:], key=lambda t: (t[0], t[1]))
        start = best[1] - MIN_K + 1
        if start != last_found:
            out.append((best[0], start))
        last_found = start
    return out


def mega_windows_of(T, c, rb, re):
    """(first_w, last_w) of a read [rb, re) (contig-local) of contig c: the mega-windows among the regions it touches"""
    borders = T.start[int(T.reg_base[c]):int(T.reg_base[c + 1])]
    bl = [int(x) for x in borders]
    first = bisect.bisect_right(bl, rb) - 1                # borders <= rb, less one: the region rb lies in
    last = bisect.bisect_left(bl, re)                      # borders < re
    even = bool(T.win_even[c])
    first_w = first if (first % 2 == 0) == even else first + 1
    last_w = last if (last % 2 == 0) == even else last - 1
    return first_w, last_w


def minimizer_votes(tables, rb, re, qae, seq_off, reads2, read_contig, wide=False):
    """(coverage, support) of every entry of the tables.  wide = True keeps num_cbases and c_dist + 3K at 32 bits where the
    reference truncates them to 16: only there to show that a read spanning more than 65 535 bases is told apart."""
    T = tables
    n_ent = int(T.mw_off[T.n_info])
    cov = [0] * n_ent
    sup = [0] * n_ent
    wmask = U32 if wide else U16
    for a in range(len(rb)):
        c = int(read_contig[a])
        base = int(T.contig_base[c])
        b, e = int(rb[a]) - base, int(re[a]) - base
        first_w, last_w = mega_windows_of(T, c, b, e)
        if last_w < first_w:
            continue
        found = {}
        for key, start in read_minimizers(read_bases(reads2, int(seq_off[a]), int(qae[a]))):
            found.setdefault(key, []).append(start)
        num_cbases = (e - b) & wmask
        even = bool(T.win_even[c])
        for w in range(first_w, last_w + 1, 2):
            x = int(T.info_base[c]) + (w // 2 if even else (w - 1) // 2)
            e0, e1 = int(T.mw_off[x]), int(T.mw_off[x + 1])
            if e0 == e1:
                continue                                    # (an empty mega-window: its border is not looked at)
            pos = int(T.start[int(T.reg_base[c]) + w])
            for m in range(e0, e1):
                pos += int(T.rel_pos[m])
                if b <= pos < e:
                    c_dist = pos - b
                    left = c_dist - 2 * MIN_K if c_dist > 2 * MIN_K else 0
                    right = min(num_cbases, (c_dist + 3 * MIN_K) & wmask)
                    cov[m] += 1
                    for s in found.get(int(T.minimisers[m]), ()):
                        if left <= s <= right:
                            sup[m] += 1
                if pos >= e:
                    break
    return np.array(cov, dtype=np.uint32), np.array(sup, dtype=np.uint32)
