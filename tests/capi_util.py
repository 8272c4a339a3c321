"""What the tests that call the C-ABI through ctypes share: the HypoArmsReads and HypoMegaWindows structs and a small set of exact-copy reads."""
import ctypes as C

import numpy as np


class ArmsReads(C.Structure):                      # HypoArmsReads, include/hypo_gpu.h
    _fields_ = [("n_alignments", C.c_uint32), ("rb", C.c_void_p), ("re", C.c_void_p), ("qae", C.c_void_p), ("seq_off", C.c_void_p),
                ("reads2", C.c_void_p), ("reads2_bytes", C.c_uint64), ("cigar_off", C.c_void_p), ("cigar", C.c_void_p), ("file_rank", C.c_void_p)]


class MegaWindows(C.Structure):                   # HypoMegaWindows, include/hypo_gpu.h
    _fields_ = [("n_contigs", C.c_uint32), ("contig_base", C.c_void_p), ("reg_base", C.c_void_p), ("win_even", C.c_void_p), ("info_base", C.c_void_p),
                ("start", C.c_void_p), ("n_info", C.c_uint32), ("mw_off", C.c_void_p), ("rel_pos", C.c_void_p), ("minimisers", C.c_void_p)]


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def exact_reads(codes, n_reads, read_len, rng):
    """n_reads exact copies of stretches of the contig, sorted by start: (rb, re, qae, seq_off, reads2, cigar_off, cigar)."""
    n = codes.size
    rb = np.sort(rng.integers(0, n - read_len, size=n_reads)).astype(np.uint32)
    keep = np.array([bool((codes[b:b + read_len] < 4).all()) for b in rb])       # (a read over an N would not pack in 2 bits)
    rb = rb[keep]
    m = rb.size
    nb = (read_len + 3) // 4
    reads2 = np.zeros(m * nb, dtype=np.uint8)
    for i, b in enumerate(rb):
        c = np.concatenate([codes[b:b + read_len], np.zeros((-read_len) % 4, np.uint8)]).reshape(-1, 4)
        reads2[i * nb:(i + 1) * nb] = (c[:, 0] << 6) | (c[:, 1] << 4) | (c[:, 2] << 2) | c[:, 3]
    re = (rb + read_len).astype(np.uint32)
    qae = np.full(m, read_len, dtype=np.uint32)
    seq_off = (np.arange(m, dtype=np.uint64) * nb).astype(np.uint64)
    cigar_off = np.arange(m + 1, dtype=np.uint32)
    cigar = np.full(m, (read_len << 4) | 0, dtype=np.uint32)
    return rb, re, qae, seq_off, reads2, cigar_off, cigar


class ArmsRegions(C.Structure):                    # HypoArmsRegions
    _fields_ = [("n_regions", C.c_uint32), ("start", C.c_void_p), ("type", C.c_void_p), ("info", C.c_void_p), ("n_anchor_kmers", C.c_uint64),
                ("anchor_kmers", C.c_void_p), ("k", C.c_uint32), ("contig4", C.c_void_p)]


class ArmsSummary(C.Structure):                    # HypoArmsSummary
    _fields_ = [("n_windows", C.c_uint32), ("n_arms", C.c_uint32), ("arms2_bytes", C.c_uint64), ("draft4_bytes", C.c_uint64), ("out_bytes", C.c_uint64)]
