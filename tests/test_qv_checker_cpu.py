"""CPU: tests/qv_checker.py itself, against a brute-force set of substrings on small inputs, and a few values worked out by hand."""
import gzip
import math

import numpy as np
import pytest

import qv_checker as qc

COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


def brute_windows(seq, k):
    """canonical k-mers (as strings) of the windows of `seq` that hold ACGTacgt only, with repeats"""
    s = seq.decode() if isinstance(seq, (bytes, bytearray)) else seq
    out = []
    for i in range(len(s) - k + 1):
        w = s[i:i + k].upper()
        if all(c in "ACGT" for c in w):
            r = "".join(COMP[c] for c in reversed(w))
            out.append(min(w, r))                 # A < C < G < T: string order is code order
    return out


def encode(w):
    v = 0
    for c in w:
        v = (v << 2) | CODE[c]
    return v


def brute_set(records, k):
    return {w for r in records for w in brute_windows(r, k)}


def check(records, queries, k):
    R = qc.read_set([r if isinstance(r, bytes) else r.encode() for r in records], k)
    want = brute_set(records, k)
    assert R.dtype == np.uint64 and R.tolist() == sorted(encode(w) for w in want)
    for q in queries:
        ws = brute_windows(q, k)
        assert qc.seq_stats(q, k, R) == (len(ws), sum(w not in want for w in ws)), q
    return R


def rnd(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(list(alphabet), n))


@pytest.mark.parametrize("k", [12, 15, 16, 21, 22, 31])
def test_against_substrings(k):
    rng = np.random.default_rng(k)
    reads = [rnd(rng, 80) for _ in range(30)]
    reads += [rnd(rng, 60, "ACGTN"), rnd(rng, 70, "ACGTRYKM"), rnd(rng, 90).lower(), rnd(rng, 50, "ACGTacgtn")]
    reads += [rnd(rng, k - 1), rnd(rng, k), "", "N" * 40, "A" * 50, "AC" * 30]
    reads += [rnd(rng, k - 1) + "N" + rnd(rng, k - 1)]                     # runs shorter than k on both sides of a break
    genome = "".join(reads[:10])
    mutated = list(genome)
    for p in range(7, len(mutated), 53):
        mutated[p] = "ACGT"[("ACGT".index(mutated[p]) + 1) % 4]
    queries = [genome, "".join(mutated), rnd(rng, 300), rnd(rng, k - 1), "", "acgtn" * 20, reads[0][5:5 + k], "T" * 50, "GT" * 30]
    check(reads, queries, k)


@pytest.mark.parametrize("k", [12, 16, 22])
def test_palindromes_at_even_k(k):
    half = "ACGTTGCAAGCT"[:k // 2]
    pal = half + "".join(COMP[c] for c in reversed(half))                # its own reverse complement
    assert len(pal) == k and brute_windows(pal, k) == [pal]
    R = check([pal + "N" + "G" * k], [pal, pal.lower(), "C" * k, pal[1:] + "A"], k)
    assert R.size == 2
    assert qc.seq_stats(pal, k, R) == (1, 0) and qc.seq_stats("C" * k, k, R) == (1, 0)      # poly-C is the reverse of poly-G


def test_a_kmer_never_spans_two_records():
    k = 12
    a, b = "ACGTACGGTCAT", "TTGACCAGTAGG"
    R = qc.read_set([a.encode()[:8], a.encode()[8:] + b.encode()], k)
    assert qc.seq_stats(a, k, R) == (1, 1) and qc.seq_stats(b, k, R) == (1, 0)


def test_files(tmp_path):
    k = 15
    rng = np.random.default_rng(5)
    reads = [rnd(rng, 100, "ACGTN") for _ in range(40)]
    want = qc.read_set([r.encode() for r in reads], k).tolist()
    fa = tmp_path / "r.fa"
    fa.write_text("".join(f">r{i} d\n" + "\n".join(r[j:j + 30] for j in range(0, len(r), 30)) + "\n" for i, r in enumerate(reads)))
    fq = tmp_path / "r.fq"
    fq.write_text("".join(f"@r{i}\n{r[:50]}\n{r[50:]}\n+\n{'I' * 50}\n{'I' * 50}\n" for i, r in enumerate(reads)))
    gz = tmp_path / "r.fq.gz"
    gz.write_bytes(gzip.compress(fq.read_bytes()))
    a, b = tmp_path / "a.fa", tmp_path / "b.fa.gz"
    a.write_text("".join(f">r{i}\n{r}\n" for i, r in enumerate(reads[:20])))
    b.write_bytes(gzip.compress("".join(f">r{i}\n{r}\n" for i, r in enumerate(reads[20:])).encode()))
    lst = tmp_path / "list.txt"
    lst.write_text(f"{a}\n{b}\n")
    for paths in ([str(fa)], [str(fq)], [str(gz)], ["@" + str(lst)], [str(a), str(b)]):
        assert qc.read_set(paths, k).tolist() == want


def test_hand_computed_values():
    k = 12
    read = "ACGTACGGTCATTG"                                               # 3 windows
    R = qc.read_set([read.encode()], k)
    assert R.size == 3
    assert qc.seq_stats(read, k, R) == (3, 0)
    rc = "".join(COMP[c] for c in reversed(read))
    assert qc.seq_stats(rc, k, R) == (3, 0)                                # the other strand
    assert qc.seq_stats(read[:13] + "A", k, R) == (3, 1)                   # last base changed: only the last window holds it
    assert qc.seq_stats(read[:6] + "N" + read[7:], k, R) == (0, 0)         # an N in every window
    assert qc.seq_stats(read + read, k, R) == (17, 11)                     # the 11 windows over the junction are new, with multiplicity
    assert qc.seq_stats(read[:11], k, R) == (0, 0)
    assert qc.qv_text(0, 3, k) == "inf" and qc.qv_text(0, 0, k) == "NA" and qc.qv_value(0, 0, k) is None
    assert qc.qv_text(3, 3, k) == "0.00"                                   # err = 1
    # missing / total = 1 - 0.5^12: err = 1 - (0.5^12)^(1/12) = 0.5, QV = 10 log10(2) = 3.0103
    assert qc.qv_text(4095, 4096, 12) == "3.01"
    # one in a million at k = 21: err = 1 - (1 - 1e-6)^(1/21) = 4.7619e-8 (to first order 1e-6 / 21): QV = 73.22
    assert qc.qv_text(1, 1000000, 21) == "73.22"
    assert abs(qc.qv_value(1, 1000000, 21) - (-10 * math.log10(1e-6 / 21))) < 1e-4
    assert qc.draft_text(b"acgtNnRyACGT-") == "ACGTNNNNACGTN"


def test_table_round_trip():
    k = 12
    read = "ACGTACGGTCATTG"
    R = qc.read_set([read.encode()], k)
    drafts = [("c1", read[:13] + "a"), ("c2", "ACGT"), ("c3", read.lower())]
    polished = [("c1", read), ("c2", ""), ("c3", read + "TTTT")]
    rws = qc.rows(drafts, polished, k, R)
    assert rws == [("c1", 1, 3, 0, 3), ("c2", 0, 0, 0, 0), ("c3", 0, 3, 4, 7), ("*", 1, 6, 4, 10)]
    text = qc.table(rws, k)
    assert text.split("\n")[2] == "c2\t0\t0\tNA\t0\t0\tNA" and text.split("\n")[1].endswith("\t0\t3\tinf")
    assert [r[:3] + r[4:6] for r in qc.parse_table(text)] == rws
