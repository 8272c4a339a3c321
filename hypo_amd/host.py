"""ctypes binding of libhypo_host.so: the C++ host mirror of the reference's object surface
(hypo_amd/csrc/host: PackedSeq, Filter, Window, Contig scan).  Used by tests; a C++ host links the mirror directly."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "_build", "libhypo_host.so")


class HostMirror:
    def __init__(self):
        from . import capi
        capi.load_library()                   # torch + libhypo_gpu first: one HIP runtime per process
        self.lib = C.CDLL(LIB_PATH)

    @staticmethod
    def _arr(strings):
        return (C.c_char_p * max(len(strings), 1))(*[s.encode() for s in strings])

    def set_scores(self, scores):
        self.lib.hypo_host_set_scores((C.c_int8 * 6)(*scores))

    def filter(self, draft, arms):
        good = (C.c_ubyte * max(len(arms), 1))()
        self.lib.hypo_host_filter(draft.encode(), C.c_int(len(arms)), self._arr(arms), good)
        return [int(x) for x in good][:len(arms)]

    def read_fastx(self, path, line_by_line=False, cap=1 << 24):
        """[(name, sequence)] of a FASTA / FASTQ file through SeqIO.hpp's reader (the mapped, parallel one unless line_by_line)"""
        out = C.create_string_buffer(cap)
        r = self.lib.hypo_host_read_fastx(str(path).encode(), C.c_int(1 if line_by_line else 0), out, C.c_int(cap))
        if r < 0:
            return None
        return [tuple(l.split("\t")) for l in out.raw[:r].decode().split("\n")[:-1]]

    def pack_roundtrip(self, nb, text):
        out = C.create_string_buffer(len(text) + 8)
        r = self.lib.hypo_host_pack_roundtrip(C.c_int(nb), text.encode(), out, C.c_int(len(text) + 8))
        return out.raw[:r].decode()

    def windows(self, wins, batched=True):
        """wins: list of hypo_amd.TextWindow (LONG windows with UNFILTERED arms).  Returns (consensus list, kept flags)."""
        n = len(wins)
        arms = []
        for w in wins:
            arms += list(w.internal) + list(w.prefix) + list(w.suffix)
        iarr = lambda xs: (C.c_int * max(n, 1))(*xs)
        cap = 4 * sum(len(w.draft) for w in wins) + 2 * sum(len(a) for a in arms) + 1024
        out = C.create_string_buffer(cap)
        lens = (C.c_int * max(n, 1))()
        kept = (C.c_ubyte * max(len(arms), 1))()
        rc = self.lib.hypo_host_windows(C.c_int(n), iarr([1 if w.is_long else 0 for w in wins]),
                                        self._arr([w.draft for w in wins]), iarr([len(w.internal) for w in wins]),
                                        iarr([len(w.prefix) for w in wins]), iarr([len(w.suffix) for w in wins]),
                                        iarr([w.n_empty for w in wins]), self._arr(arms), out, C.c_long(cap), lens, kept,
                                        C.c_int(1 if batched else 0))
        if rc != 0:
            raise RuntimeError(f"hypo_host_windows rc={rc}")
        cons, o = [], 0
        for i in range(n):
            cons.append(out.raw[o:o + lens[i]].decode())
            o += lens[i]
        return cons, [int(x) for x in kept][:len(arms)]

    def contig_scan(self, seq, k, words, rank_q, sel_q):
        ns = C.c_uint64(0)
        kids = np.zeros(max(len(seq), 1), dtype=np.uint64)
        rq = np.asarray(rank_q, dtype=np.uint64); ra = np.zeros(max(rq.size, 1), dtype=np.uint64)
        sq = np.asarray(sel_q, dtype=np.uint64); sa = np.zeros(max(sq.size, 1), dtype=np.uint64)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        rc = self.lib.hypo_host_contig_scan(seq.encode(), C.c_uint(k), p(words), C.c_uint64(words.size), C.byref(ns),
                                            p(kids), C.c_uint64(kids.size), p(rq), p(ra), C.c_int(rq.size), p(sq), p(sa),
                                            C.c_int(sq.size))
        if rc != 0:
            raise RuntimeError(f"hypo_host_contig_scan rc={rc}")
        n = int(ns.value)
        return n, kids[:n], ra[:rq.size], sa[:sq.size]

    def plan_contexts(self, initial_cid, final_cid, n_ctx, n_reads, contig_len, split_batch, allow_pieces):
        """[(c0, c1, piece, own0, own1)] per device context: how Hypo::polish deals the contigs [initial_cid, final_cid) of a batch out
        (host/CtxPlan.hpp); n_reads and contig_len per contig of the batch"""
        nr = np.asarray(n_reads, dtype=np.uint64)
        cl = np.asarray(contig_len, dtype=np.uint32)
        assert nr.size == cl.size == final_cid - initial_cid and n_ctx >= 1
        out = np.zeros(5 * n_ctx, dtype=np.uint32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        self.lib.hypo_host_plan_contexts(C.c_uint32(initial_cid), C.c_uint32(final_cid), C.c_int(n_ctx), p(nr), p(cl),
                                         C.c_int(1 if split_batch else 0), C.c_int(1 if allow_pieces else 0), p(out))
        return [(int(r[0]), int(r[1]), bool(r[2]), int(r[3]), int(r[4])) for r in out.reshape(n_ctx, 5)]

    def kmer_votes(self, k, total_len, spos, kids, rb, re, qae, seq_off, reads2):
        """(coverage, support) of Alignment::update_solidkmers_support over every read: the host loop on the flat arrays
        hypo_gpu_reads_upload / hypo_gpu_support_kmers take (include/hypo_gpu.h)"""
        spos = np.ascontiguousarray(spos, dtype=np.uint32); kids = np.ascontiguousarray(kids, dtype=np.uint64)
        rb, re, qae = (np.ascontiguousarray(x, dtype=np.uint32) for x in (rb, re, qae))
        seq_off = np.ascontiguousarray(seq_off, dtype=np.uint64); reads2 = np.ascontiguousarray(reads2, dtype=np.uint8)
        cov = np.zeros(max(spos.size, 1), dtype=np.uint32); sup = np.zeros(max(spos.size, 1), dtype=np.uint32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        rc = self.lib.hypo_host_kmer_votes(C.c_uint32(k), C.c_uint64(total_len), C.c_uint64(spos.size), p(spos), p(kids), C.c_uint32(rb.size),
                                           p(rb), p(re), p(qae), p(seq_off), p(reads2), p(cov), p(sup))
        if rc != 0:
            raise RuntimeError(f"hypo_host_kmer_votes rc={rc}")
        return cov[:spos.size], sup[:spos.size]

    def minimizer_votes(self, tables, rb, re, qae, seq_off, reads2, read_contig):
        """(coverage, support) of Alignment::update_minimisers_support over every read; tables: the arrays of HypoMegaWindows by
        name (contig_base, reg_base, win_even, info_base, start, n_info, mw_off, rel_pos, minimisers)"""
        u32 = lambda a: np.ascontiguousarray(a, dtype=np.uint32)
        T = tables
        cb, rbase, ib, start, off, rel, mins = (u32(x) for x in (T.contig_base, T.reg_base, T.info_base, T.start, T.mw_off, T.rel_pos, T.minimisers))
        even = np.ascontiguousarray(T.win_even, dtype=np.uint8)
        rb, re, qae, ctg = (u32(x) for x in (rb, re, qae, read_contig))
        seq_off = np.ascontiguousarray(seq_off, dtype=np.uint64); reads2 = np.ascontiguousarray(reads2, dtype=np.uint8)
        n_ent = int(off[T.n_info])
        cov = np.zeros(max(n_ent, 1), dtype=np.uint32); sup = np.zeros(max(n_ent, 1), dtype=np.uint32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        rc = self.lib.hypo_host_minimizer_votes(C.c_uint32(cb.size), p(cb), p(rbase), p(even), p(ib), p(start), C.c_uint32(T.n_info), p(off), p(rel), p(mins),
                                                C.c_uint32(rb.size), p(rb), p(re), p(qae), p(seq_off), p(reads2), p(ctg), p(cov), p(sup))
        if rc != 0:
            raise RuntimeError(f"hypo_host_minimizer_votes rc={rc}")
        return cov[:n_ent], sup[:n_ent]

    def _arms(self, long_mode, regions, reads):
        u32 = lambda a: np.ascontiguousarray(a, dtype=np.uint32)
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        nr = int(regions.n_regions)
        start, rtype, contig4 = u32(regions.start), np.ascontiguousarray(regions.type, dtype=np.uint8), np.ascontiguousarray(regions.contig4, dtype=np.uint8)
        rb, re, qae, cigar_off, cigar = (u32(x) for x in (reads.rb, reads.re, reads.qae, reads.cigar_off, reads.cigar))
        seq_off = np.ascontiguousarray(reads.seq_off, dtype=np.uint64); reads2 = np.ascontiguousarray(reads.reads2, dtype=np.uint8)
        rank = None if getattr(reads, "file_rank", None) is None else u32(reads.file_rank)
        valid = np.zeros(nr, dtype=np.uint8); counts = np.zeros(4 * nr, dtype=np.uint32)
        cap = int(start[nr]) + 2 * int(qae.sum()) + 8 * int(rb.size) + nr + 1024
        text = C.create_string_buffer(cap)
        tail = (C.c_uint32(rb.size), p(rb), p(re), p(qae), p(seq_off), p(reads2), p(cigar_off), p(cigar), p(rank), p(valid), p(counts), text, C.c_long(cap))
        if long_mode:
            f = self.lib.hypo_host_long_arms
            f.restype = C.c_long
            n = f(C.c_uint32(nr), p(start), p(rtype), p(contig4), *tail)
        else:
            info, anchors = u32(regions.info), np.ascontiguousarray(regions.anchor_kmers, dtype=np.uint64)
            f = self.lib.hypo_host_short_arms
            f.restype = C.c_long
            n = f(C.c_uint32(nr), p(start), p(rtype), p(info), C.c_uint64(anchors.size), p(anchors), C.c_uint32(regions.k), p(contig4), *tail)
        if n < 0:
            raise RuntimeError(f"hypo_host_{'long' if long_mode else 'short'}_arms rc={n}")
        return valid, counts.reshape(nr, 4), text.raw[:n].decode().split("\n")[:-1]

    def short_arms(self, regions, reads):
        """Alignment::find_short_arms of every record in file order (reads.file_rank, or the order given) + Contig::fill_short_windows over
        the flat arrays hypo_gpu_arms_build takes (attributes named as in HypoArmsRegions / HypoArmsReads): (valid [n_regions], internal /
        prefix / suffix / empty [n_regions, 4], Window::dump_text of every remaining window in region order)"""
        return self._arms(False, regions, reads)

    def long_arms(self, regions, reads):
        """the same through Alignment::find_long_arms + Contig::fill_long_windows over pseudo regions (SR / LONG)"""
        return self._arms(True, regions, reads)
