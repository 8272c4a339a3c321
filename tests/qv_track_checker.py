"""CPU checker of `hypo --qv-bed` and hypo_gpu_kset_query_track (DESIGN.md "k-mer QV track"): the contract in plain numpy on top
of qv_checker.  It shares no code with the host library or the kernels.

k, R, the byte rules and the windows are those of qv_checker.  Window i of a sequence S is MISSING when S[i, i + k) is all
ACGTacgt and its canonical k-mer is not in R.  A base is COVERED when a missing window contains it; the INTERVALS of S are the
maximal runs [start, end) of covered bases, so missing windows that overlap or abut share one, end - start >= k, and
start[j + 1] > end[j].  n of an interval = the missing windows that start in [start, end - k]; they add up to seq_stats' missing.
Intervals belong to one sequence: nothing joins two of them.

  missing_starts(seq, k, R)        the starts of the missing windows, ascending (i64 array)
  intervals(seq, k, R)             [(start, end, n)]
  track(seqs, k, R, want=None)     (total, missing, iv_off, iv_start, iv_end, iv_missing) as the entry point returns them
  bed(contigs, k, R)               the file `hypo --qv-bed` writes; contigs: [(name, text)] in draft order
  parse_bed(text)                  [(name, start, end, n)]
"""
import numpy as np

import qv_checker as qc

HEADER = "#contig\tstart\tend\tmissing_kmers"


def missing_starts(seq, k, R):
    seq = seq.encode() if isinstance(seq, str) else bytes(seq)
    codes = qc._LUT[np.frombuffer(seq, dtype=np.uint8)]
    n = codes.size - k + 1
    if n <= 0:
        return np.zeros(0, np.int64)
    bad = np.concatenate([[0], np.cumsum(codes > 3)])
    starts = np.flatnonzero((bad[k:k + n] - bad[:n]) == 0)              # the windows made of bases only, in order
    w = qc.canonical_windows(seq, k)
    assert w.size == starts.size
    if R.size == 0:
        return starts
    at = np.minimum(np.searchsorted(R, w), R.size - 1)
    return starts[R[at] != w]


def intervals(seq, k, R):
    p = missing_starts(seq, k, R)
    if p.size == 0:
        return []
    first = np.flatnonzero(np.concatenate([[True], np.diff(p) > k]))    # a start more than k behind the one before opens an interval
    last = np.concatenate([first[1:], [p.size]]) - 1
    return [(int(p[a]), int(p[b]) + k, int(b - a + 1)) for a, b in zip(first, last)]


def track(seqs, k, R, want=None):
    total, missing, iv_off, rows = [], [], [0], []
    for s, seq in enumerate(seqs):
        t, m = qc.seq_stats(seq, k, R)
        total.append(t)
        missing.append(m)
        if want is None or want[s]:
            rows += intervals(seq, k, R)
        iv_off.append(len(rows))
    cols = [[r[i] for r in rows] for i in range(3)]
    return total, missing, iv_off, cols[0], cols[1], cols[2]


def bed(contigs, k, R):
    lines = [HEADER]
    for name, text in contigs:
        lines += [f"{name}\t{a}\t{b}\t{n}" for a, b, n in intervals(text, k, R)]
    return "\n".join(lines) + "\n"


def parse_bed(text):
    lines = text.split("\n")
    assert lines[0] == HEADER and lines[-1] == ""
    out = []
    for l in lines[1:-1]:
        f = l.split("\t")
        assert len(f) == 4, l
        out.append((f[0], int(f[1]), int(f[2]), int(f[3])))
    return out
