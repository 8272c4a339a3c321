"""CPU checker of `hypo --qv-min-count` (DESIGN.md "k-mer min count"): the contract in plain Python / numpy.  It shares no code with
the host library or the kernels.

The flag changes one thing: wherever `--qv`, `--qv-bed`, `--kmer-guard` and `--guard-records` ask whether a k-mer is "in R", the set
of the canonical k-mers of the reads, they ask whether it is in R_t = { x : count(x) >= t }, count(x) = the length-k windows of the
reads with canonical k-mer x, stopping at 255.  So this checker only makes R_t and t; qv_checker, qv_track_checker, guard_checker and
guard_records_checker take R as a sorted key array and are called with R_t in its place, unchanged.

  read_counts(paths_or_seqs, k)   (keys, counts): sorted distinct canonical k-mers (u64) and their window counts, stopping at 255.
                                  The byte rules are those of qv_checker: ACGTacgt are bases, any other byte or a record end ends a
                                  run; every window counts once, a palindromic one too.
  histogram(counts)               h[c], c = 0..255: the distinct k-mers with count c (h[0] = 0)
  threshold(h, given)             t: `given` when it is an integer 1..255; for "valley" the smallest c in 2..254 with h[c] <= h[c + 1],
                                  2 when there is none
  reliable_set(keys, counts, t)   R_t as a sorted u64 array; R_1 is `keys`
  info_line(k, h, given)          the line `hypo` prints on stdout after the reads' pass (t >= 2 only)
"""
import numpy as np

import qv_checker as qc
import solid_checker as sc

CAP = 255


def _records(paths_or_seqs):
    if isinstance(paths_or_seqs, (bytes, bytearray)):
        return [bytes(paths_or_seqs)]
    if isinstance(paths_or_seqs, (list, tuple)) and (not paths_or_seqs or isinstance(paths_or_seqs[0], (bytes, bytearray))):
        return list(paths_or_seqs)
    return sc.parse_records(paths_or_seqs)


def read_counts(paths_or_seqs, k):
    recs = _records(paths_or_seqs)
    keys, counts = np.zeros(0, np.uint64), np.zeros(0, np.int64)
    for i in range(0, len(recs), 4096):
        u, c = np.unique(qc.canonical_windows(b"\n".join(recs[i:i + 4096]), k), return_counts=True)
        keys, inv = np.unique(np.concatenate([keys, u]), return_inverse=True)
        counts = np.bincount(inv, weights=np.concatenate([counts, c.astype(np.int64)]), minlength=keys.size).astype(np.int64)
    return keys, np.minimum(counts, CAP)


def histogram(counts):
    return np.bincount(np.asarray(counts, np.int64), minlength=CAP + 1)[:CAP + 1]


def threshold(h, given):
    if given != "valley":
        t = int(given)
        assert 1 <= t <= CAP
        return t
    for c in range(2, CAP):
        if h[c] <= h[c + 1]:
            return c
    return 2


def reliable_set(keys, counts, t):
    assert 1 <= t <= CAP
    return np.asarray(keys, np.uint64)[np.asarray(counts) >= t]


def info_line(k, h, given):
    t = threshold(h, given)
    return (f"[Hypo::Hypo] Info: k-mer min count (k = {k}): >= {t} ({'valley' if given == 'valley' else 'given'}), "
            f"{int(np.asarray(h)[t:].sum())} of {int(np.asarray(h).sum())} read k-mers reliable")
