"""CPU: the checker of the solid k-mer construction (tests/solid_checker.py) on hand-made inputs whose answers are worked out by
hand in the comments: the parsing and counting contract of DESIGN.md "Solid k-mers from the reads"."""
import gzip

import numpy as np

import solid_checker as sc

A, C, G, T = 0, 1, 2, 3


def code(s):
    v = 0
    for ch in s:
        v = (v << 2) | "ACGT".index(ch)
    return v


def counts_of(seqs, k):
    codes, counts = sc.count_canonical(seqs, k)
    return {int(c): int(n) for c, n in zip(codes, counts)}


def test_canonical_is_min_of_both_strands():
    # ACG (6) and its reverse complement CGT (27): both count on ACG
    assert counts_of([b"ACG", b"CGT"], 3) == {code("ACG"): 2}
    assert sc.revcomp_codes([code("AAC")], 3)[0] == code("GTT")


def test_non_bases_break_runs_and_lower_case_counts():
    # N and IUPAC R split the read: "acgt" + "ACG" -> ACG, CGT (= ACG) in the first, ACG in the second
    assert counts_of([b"acgtNACG"], 3) == {code("ACG"): 3}
    assert counts_of([b"ACGRACG"], 3) == {code("ACG"): 2}
    # a k-mer never spans two records
    assert counts_of([b"AC", b"GT"], 3) == {}


def test_reads_shorter_than_k():
    assert counts_of([b"ACGT", b"AC", b""], 5) == {}


def test_even_k_palindrome_is_one_kmer():
    # ACGT is its own reverse complement: counted once per occurrence
    assert counts_of([b"ACGT", b"ACGT"], 4) == {code("ACGT"): 2}
    codes, counts = np.array([code("ACGT")], np.uint64), np.array([3])
    words, n_bits, n_can = sc.solid_set(codes, counts, 4, 30, 2, 120, exclude_hp=True)
    assert (n_bits, n_can) == (1, 1) and int(words[0]) == 1 << code("ACGT")


def test_homopolymer_rule_and_both_strands():
    k = 5
    codes = np.array([code("AACGT"), code("ACGTT"), code("ACGTC")], np.uint64)   # hp at the start, hp at the end, none
    counts = np.array([5, 5, 5])
    words, n_bits, n_can = sc.solid_set(codes, counts, k, 30, 2, 120)
    assert (n_bits, n_can) == (2, 1)
    bits = {i for i in range(1 << (2 * k)) if (int(words[i >> 6]) >> (i & 63)) & 1}
    assert bits == {code("ACGTC"), code("GACGT")}


def test_kmc_filters_and_cutoff_window():
    codes = np.array([code("ACGTC"), code("ACGAC"), code("CAGTC"), code("CTGAC")], np.uint64)
    counts = np.array([1, 2, 120, 121])                  # -ci2 drops 1, -cx120 (c = 30) drops 121
    h = sc.histogram(counts, 30)
    assert h.size == 121 and h[1] == 0 and h[2] == 1 and h[120] == 1 and h.sum() == 2
    _, _, n_can = sc.solid_set(codes, counts, 5, 30, 2, 1000)
    assert n_can == 2
    _, _, n_can = sc.solid_set(codes, counts, 5, 30, 3, 119)
    assert n_can == 0


def test_formats(tmp_path):
    # multi-line FASTA, FASTQ (a quality line may start with '@' or '+'), gzip, CRLF and an @list give the same records
    (tmp_path / "a.fa").write_bytes(b">r1 desc\nACGT\nAC\n\n>r2\r\nGGNA\r\n")
    (tmp_path / "b.fq").write_bytes(b"@r1\nACGTAC\n+\n@+IIII\n@r2\nGGNA\n+r2\nIIII\n")
    (tmp_path / "c.fq.gz").write_bytes(gzip.compress((tmp_path / "b.fq").read_bytes()))
    (tmp_path / "list").write_text(f"{tmp_path / 'a.fa'}\n\n{tmp_path / 'c.fq.gz'}\n")
    want = [b"ACGTAC", b"GGNA"]
    assert sc.parse_records([str(tmp_path / "a.fa")]) == want
    assert sc.parse_records([str(tmp_path / "b.fq")]) == want
    assert sc.parse_records([str(tmp_path / "c.fq.gz")]) == want
    assert sc.parse_records(sc.expand_paths("@" + str(tmp_path / "list"))) == want + want


def test_undefined_histogram_and_degenerate_reads():
    out = sc.build([b"ACGT"], 5, 30)
    assert out["cut"] is None and "words" not in out
    assert sc.find_cutoffs([0, 0, 9, 4, 1, 0, 0]) is None


def test_whole_contract_small():
    # 40 copies of a 30-base read among 250 random ones: the cut-offs exist, and every kept canonical k-mer without a homopolymer
    # end is set on both strands
    rng = np.random.default_rng(1)
    read = bytes(rng.choice(list(b"ACGT"), 30).astype(np.uint8))
    noise = [bytes(rng.choice(list(b"ACGT"), 30).astype(np.uint8)) for _ in range(200)]
    out = sc.build([read] * 40 + noise + noise[:50], 11, 30)
    assert out["cut"] is not None
    err, mean, lower, upper = out["cut"]
    words = out["words"]
    c = out["codes"][(out["counts"] >= lower) & (out["counts"] <= upper) & (out["counts"] >= 2)]
    for x in c:
        s = "".join("ACGT"[(int(x) >> (2 * (10 - i))) & 3] for i in range(11))
        if s[0] != s[1] and s[-1] != s[-2]:
            r = int(sc.revcomp_codes([x], 11)[0])
            assert (int(words[int(x) >> 6]) >> (int(x) & 63)) & 1 and (int(words[r >> 6]) >> (r & 63)) & 1
