"""CPU checker of `hypo --qv` (DESIGN.md "k-mer QV"): the whole contract in plain Python / numpy, from the read files to the
table.  It shares no code with the host library or the kernels.

  read_set(paths_or_seqs, k)   R: the canonical k-mers (min(fwd, rc), A0 C1 G2 T3, MSB-first) of all records, as a sorted u64
                               array.  Files follow DESIGN 3.5 (FASTA / FASTQ, plain, gzip or "@list"); ACGTacgt are bases, any
                               other byte ends a run, no k-mer spans two records.  Presence only: seen once is in R.
  seq_stats(seq, k, R)         (total, missing) of one sequence: its length-k windows made of ACGTacgt only, and those of them,
                               counted with multiplicity, whose canonical k-mer is not in R
  qv_value / qv_text           err = 1 - (1 - missing / total)^(1 / k), QV = -10 log10(err); "inf" when nothing is missing, "NA"
                               when there is no window; "%.2f" otherwise
  draft_text(seq)              a draft contig as PackedSeq::base_at gives it: ACGT upper case, every other byte N
  table(...)                   the file `hypo --qv` writes
"""
import math

import numpy as np

import solid_checker as sc

_LUT = np.full(256, 4, dtype=np.uint8)
for _i, _ch in enumerate(b"ACGT"):
    _LUT[_ch] = _i
    _LUT[_ch | 0x20] = _i

HEADER = "#contig\tdraft_missing\tdraft_total\tdraft_qv\tpolished_missing\tpolished_total\tpolished_qv"


def canonical_windows(seq, k):
    """the canonical code of every length-k window of `seq` that holds bases only, in order (u64 array, with repeats)"""
    assert 1 <= k <= 31
    b = _LUT[np.frombuffer(bytes(seq), dtype=np.uint8)]
    n = b.size - k + 1
    if n <= 0:
        return np.zeros(0, np.uint64)
    bad = np.concatenate([[0], np.cumsum(b > 3)])
    ok = (bad[k:k + n] - bad[:n]) == 0
    c = np.minimum(b, 3).astype(np.uint64)
    fwd = np.zeros(n, dtype=np.uint64)
    rc = np.zeros(n, dtype=np.uint64)
    for j in range(k):
        fwd = (fwd << np.uint64(2)) | c[j:j + n]
        rc |= (np.uint64(3) - c[j:j + n]) << np.uint64(2 * j)
    return np.minimum(fwd, rc)[ok]


def read_set(paths_or_seqs, k):
    if isinstance(paths_or_seqs, (bytes, bytearray)):
        seqs = [bytes(paths_or_seqs)]
    elif isinstance(paths_or_seqs, (list, tuple)) and (not paths_or_seqs or isinstance(paths_or_seqs[0], (bytes, bytearray))):
        seqs = list(paths_or_seqs)
    else:
        seqs = sc.parse_records(paths_or_seqs)
    parts = [np.unique(canonical_windows(b"\n".join(seqs[i:i + 4096]), k)) for i in range(0, len(seqs), 4096)]
    return np.unique(np.concatenate(parts)) if parts else np.zeros(0, np.uint64)


def seq_stats(seq, k, R):
    w = canonical_windows(seq.encode() if isinstance(seq, str) else seq, k)
    if w.size == 0:
        return 0, 0
    if R.size == 0:
        return int(w.size), int(w.size)
    at = np.minimum(np.searchsorted(R, w), R.size - 1)
    return int(w.size), int(np.count_nonzero(R[at] != w))


def qv_value(missing, total, k):
    """None for NA, math.inf for no missing k-mer"""
    if total == 0:
        return None
    if missing == 0:
        return math.inf
    err = 1.0 - (1.0 - missing / total) ** (1.0 / k)
    return -10.0 * math.log10(err) + 0.0


def qv_text(missing, total, k):
    v = qv_value(missing, total, k)
    return "NA" if v is None else "inf" if v == math.inf else "%.2f" % v


def draft_text(seq):
    return "".join(c if c in "ACGT" else "N" for c in (seq.decode() if isinstance(seq, (bytes, bytearray)) else seq).upper())


def rows(drafts, polished, k, R):
    """[(name, dm, dt, pm, pt)] per contig and the sums as "*"; drafts / polished: [(name, sequence)] in draft order"""
    out = []
    for (name, d), (pname, p) in zip(drafts, polished):
        assert name == pname
        dt, dm = seq_stats(draft_text(d), k, R)
        pt, pm = seq_stats(p, k, R)
        out.append((name, dm, dt, pm, pt))
    out.append(("*",) + tuple(sum(r[i] for r in out) for i in range(1, 5)))
    return out


def table(rws, k):
    lines = [HEADER]
    for name, dm, dt, pm, pt in rws:
        lines.append(f"{name}\t{dm}\t{dt}\t{qv_text(dm, dt, k)}\t{pm}\t{pt}\t{qv_text(pm, pt, k)}")
    return "\n".join(lines) + "\n"


def parse_table(text):
    """[(name, dm, dt, dqv, pm, pt, pqv)] with the integers as int and the QVs as printed"""
    lines = text.split("\n")
    assert lines[0] == HEADER and lines[-1] == ""
    out = []
    for l in lines[1:-1]:
        f = l.split("\t")
        assert len(f) == 7, l
        out.append((f[0], int(f[1]), int(f[2]), f[3], int(f[4]), int(f[5]), f[6]))
    return out
