"""GPU: `hypo --kmer-bridge` end to end, on scenario() of tests/test_gpu_kmer_fix.py (the polish has no alignments on the second half of
every contig) with edits planted in the draft where no kept alignment reaches: insertions and deletions of 2 to 6 bases and pairs of
substitutions 2 to 10 apart, at a fixed seed, 160 bases apart, every inserted base matched by a deleted one so that the contigs keep
their lengths and the SAM headers stay true.  For every set the run without the flag gives the base FASTA and stdout; with the flag
the FASTA is the checker's (tests/kmer_bridge_checker.py) over the base FASTA, the TSV is the checker's text and applied backwards
turns the new FASTA into the base one, stdout differs by the one Info line, whose numbers are the checker's, and no .tmp is left.
Then next to the other flags.

The floors of test_bridge_pair are those the checker alone meets on the CPU stand-in's base FASTA of this scenario (DESIGN.md "k-mer
bridge" has the table): bridges that change the length by 2 or more, bridges that replace 2 or more bases by as many, and at least one
AMBIGUOUS site."""
import os
import re

import numpy as np
import pytest

import e2e_util as eu
import edit_checker as ec
import kmer_bridge_checker as kb
import kmer_fix_checker as fc
import min_count_checker as mc
import qv_checker as qc
import qv_track_checker as tc
from test_gpu_kmer_fix import check_pair as check_fix_pair, fasta_bytes, scenario
from test_gpu_qv import drop_aux, opt, run
from test_gpu_qv_bed import stable

pytestmark = pytest.mark.gpu
INFO = r"^\[Hypo::Hypo\] Info: k-mer bridge .*$"
SPACING = 160                                                              # at least 3k for every k tried


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(eu.BIN):
        eu.build_binary()


def plant(tmp_path, argv, seed=2026):
    """the draft with the planted edits in place of the draft; returns the number of edits.  A contig gets them from half its LN plus
    the longest read of the SAM files on, where there is room"""
    longest, ln = 0, {}
    for f in ("sr.sam", "lr.sam"):
        p = os.path.join(str(tmp_path), f)
        if not os.path.exists(p):
            continue
        for line in open(p):
            if line.startswith("@SQ"):
                tags = dict(t.split(":", 1) for t in line.rstrip("\n").split("\t")[1:])
                ln[tags["SN"]] = int(tags["LN"])
            elif not line.startswith("@"):
                longest = max(longest, len(line.split("\t", 10)[9]))
    rng = np.random.default_rng(seed)
    draft_path = os.path.join(str(tmp_path), opt(argv, "-d"))
    out, planted = [], 0
    for name, seq in ec.read_fastx(draft_path):
        assert ln[name] == len(seq)
        first, last = ln[name] // 2 + longest + 200, ln[name] - 200
        spots = list(range(first, last, SPACING))
        spots = spots[:len(spots) // 3 * 3]                                # whole triples: an insertion, a deletion of as many bases, a pair
        edits = []
        for i in range(0, len(spots), 3):
            n, gap = 2 + (i // 3) % 5, 2 + (i // 3) % 9
            edits.append((spots[i], 0, "".join(rng.choice(list("ACGT"), n))))
            edits.append((spots[i + 1], n, ""))
            p = spots[i + 2]
            swap = lambda c: "ACGT"[("ACGT".index(c.upper()) + 1 + int(rng.integers(3))) % 4] if c.upper() in "ACGT" else c
            edits.append((p, gap + 1, swap(seq[p]) + seq[p + 1:p + gap] + swap(seq[p + gap])))
        s = seq
        for p, gone, new in reversed(edits):
            s = s[:p] + new + s[p + gone:]
        assert len(s) == len(seq)
        planted += len(edits)
        out.append((name, s))
    assert planted >= 30
    open(draft_path, "w").write("".join(f">{n}\n{s}\n" for n, s in out))
    return planted


def planted_scenario(name, tmp_path):
    argv, out_path, reads = scenario(name, tmp_path)
    plant(tmp_path, argv)
    return argv, out_path, reads


def apply_backwards(contigs, rows):
    """the TSV's lines of every contig undone from the last to the first: the text before the pass"""
    out = []
    for name, s in contigs:
        b = bytearray(s.encode())
        mine = [r for r in rows if r[0] == name]
        shift = sum((0 if r[3] == "." else len(r[3])) - (0 if r[2] == "." else len(r[2])) for r in mine)
        for _, pos, ref, alt, _, _ in reversed(mine):
            ref, alt = ("" if x == "." else x for x in (ref, alt))
            shift -= len(alt) - len(ref)                                   # what the lines in front of this one moved it by
            assert b[pos + shift:pos + shift + len(alt)] == alt.encode()
            b[pos + shift:pos + shift + len(alt)] = ref.encode()
        out.append((name, b.decode()))
    return out


def check_pair(base_fa, new_fa, tsv_path, k, R, stdout=None, tsv_name=None, M=kb.DEFAULT_MAX, D=kb.DEFAULT_SLACK):
    """the new FASTA and the TSV against the checker run on the base FASTA; returns (rows of the TSV, the checker's stats)"""
    base = ec.read_fastx(base_fa)
    want, want_tsv, st = kb.run(base, k, R, M, D)
    got = open(new_fa, "rb").read()
    assert got == fasta_bytes(want), "the FASTA is not the checker's"
    text = open(tsv_path).read()
    assert text == want_tsv
    rows = kb.parse_tsv(text)
    new = ec.read_fastx(new_fa)
    assert fasta_bytes(apply_backwards(new, rows)) == fasta_bytes(base)
    for name, s in base:                                                   # a contig's lines applied from the last to the first give the record
        assert kb.apply(s, [r[1:] for r in rows if r[0] == name]).decode() == dict(new)[name]
    assert [r[0] for r in rows] == sorted((r[0] for r in rows), key=[n for n, _ in base].index)          # contigs in draft order
    if stdout is not None:
        info = re.findall(INFO, stdout, flags=re.M)
        assert info == [kb.info_line(tsv_name, k, M, D, st)], (info, kb.info_line(tsv_name, k, M, D, st))
    return rows, st


def lens(row):
    return (0 if row[2] == "." else len(row[2])), (0 if row[3] == "." else len(row[3]))


@pytest.mark.parametrize("name,k", [("e2e_20k_s1", None), ("e2e_20k_s1", 31), ("e2e_5ctg_long_s21", None)])
def test_bridge_pair(name, k, tmp_path):
    argv, out_path, reads = planted_scenario(name, tmp_path)
    if name == "e2e_5ctg_long_s21":
        assert opt(argv, "-p") == "2" and "-B" in argv
    kk = 21 if k is None else k
    kargs = [] if k is None else ["--qv-k", str(k)]
    R = qc.read_set([reads], kk)
    no_tmp = lambda: not [f for f in os.listdir(str(tmp_path)) if f.endswith(".tmp")]
    p0 = run(argv, tmp_path)
    assert "k-mer bridge" not in p0.stdout
    base_fa = str(tmp_path / "base.fa")
    os.rename(out_path, base_fa)
    p = run(argv + ["--kmer-bridge", "b.tsv"] + kargs, tmp_path)
    rows, st = check_pair(base_fa, out_path, str(tmp_path / "b.tsv"), kk, R, p.stdout, "b.tsv")
    assert stable(p.stdout, ["[Hypo::Hypo] Info: k-mer bridge "]) == stable(p0.stdout)
    assert len(stable(p.stdout)) == len(stable(p0.stdout)) + 1
    assert no_tmp()
    assert st.bridged == len(rows) and st.removed == sum(r[4] for r in rows)
    assert sum(1 for r in rows if abs(lens(r)[0] - lens(r)[1]) >= 2) >= 1
    assert sum(1 for r in rows if lens(r)[0] == lens(r)[1] >= 2) >= 1
    if name == "e2e_20k_s1":
        assert len(rows) >= 20 and st.ambiguous + st.over_budget >= 1, st.tuple()
    # other limits: the checker's again
    p = run(argv + ["-o", "n.fa", "--kmer-bridge", "n.tsv", "--kmer-bridge-max", "40", "--kmer-bridge-slack", "3"] + kargs, tmp_path)
    rows2, st2 = check_pair(base_fa, str(tmp_path / "n.fa"), str(tmp_path / "n.tsv"), kk, R, p.stdout, "n.tsv", 40, 3)
    assert st2.sites <= st.sites and st2.intervals == st.intervals and rows2 != rows


@pytest.mark.parametrize("name", ["e2e_20k_s1", "e2e_5ctg_long_s21"])
def test_bridge_with_the_other_flags(name, tmp_path):
    """the multi-contig set: what is per contig (--vcf, --qv, --qv-bed, -p 1); the small set: the fix, the guard, the least count and
    the stages as well"""
    argv, out_path, reads = planted_scenario(name, tmp_path)
    k = 21
    R = qc.read_set([reads], k)
    path = lambda f: str(tmp_path / f)
    no_tmp = lambda: not [f for f in os.listdir(str(tmp_path)) if f.endswith(".tmp")]
    # --vcf and --qv without and with the flag: the same VCF bytes; polished_missing drops per contig by the sum of missing_kmers
    run(argv + ["-o", "base.fa", "--vcf", "v0.vcf", "--qv", "q0.tsv"], tmp_path)
    p = run(argv + ["-o", "new.fa", "--vcf", "v1.vcf", "--qv", "q1.tsv", "--qv-bed", "b.bed", "--kmer-bridge", "b.tsv"], tmp_path)
    rows, st = check_pair(path("base.fa"), path("new.fa"), path("b.tsv"), k, R, p.stdout, "b.tsv")
    assert rows
    assert open(path("v1.vcf"), "rb").read() == open(path("v0.vcf"), "rb").read()
    t0, t1 = qc.parse_table(open(path("q0.tsv")).read()), qc.parse_table(open(path("q1.tsv")).read())
    removed = {}
    for r in rows:
        removed[r[0]] = removed.get(r[0], 0) + r[4]
    removed["*"] = sum(removed.values())
    assert [(a[0], a[1], a[2], a[3]) for a in t0] == [(b[0], b[1], b[2], b[3]) for b in t1]              # the draft columns do not move
    assert [(a[0], a[4] - b[4]) for a, b in zip(t0, t1)] == [(a[0], removed.get(a[0], 0)) for a in t0]
    new = ec.read_fastx(path("new.fa"))
    assert [(r[0], r[4], r[5]) for r in t1[:-1]] == [(n, m, t) for n, (t, m) in ((n, qc.seq_stats(s, k, R)) for n, s in new)]
    assert open(path("b.bed")).read() == tc.bed(new, k, R)
    assert no_tmp()
    tsv, new_bytes = open(path("b.tsv")).read(), open(path("new.fa"), "rb").read()
    # -p 1 writes the same files
    a1 = list(argv)
    if "-p" in a1:
        a1[a1.index("-p") + 1] = "1"
    else:
        a1 += ["-p", "1"]
    run(a1 + ["-o", "p1.fa", "--kmer-bridge", "p1.tsv"], tmp_path)
    assert open(path("p1.tsv")).read() == tsv and open(path("p1.fa"), "rb").read() == new_bytes
    if name != "e2e_20k_s1":
        return
    # with --kmer-fix: the fixes over the base text, the bridges over the fixed text, both files their checkers'
    p = run(argv + ["-o", "fb.fa", "--kmer-fix", "f.tsv", "--kmer-bridge", "fb.tsv"], tmp_path)
    fixed, fix_tsv, fix_st = fc.run(ec.read_fastx(path("base.fa")), k, R)
    open(path("fixed_by_checker.fa"), "wb").write(fasta_bytes(fixed))
    assert open(path("f.tsv")).read() == fix_tsv and fix_st.fixed >= 1
    assert re.findall(r"^\[Hypo::Hypo\] Info: k-mer fix .*$", p.stdout, flags=re.M) == [fc.info_line("f.tsv", k, fix_st)]
    check_pair(path("fixed_by_checker.fa"), path("fb.fa"), path("fb.tsv"), k, R, p.stdout, "fb.tsv")
    run(argv + ["-o", "f.fa", "--kmer-fix", "f2.tsv"], tmp_path)              # the fix alone: the bridge's input
    assert open(path("f.fa"), "rb").read() == fasta_bytes(fixed) and open(path("f2.tsv")).read() == fix_tsv
    # with the guard: the bridges are made over the guarded text, and the VCF is the guard's
    run(argv + ["-o", "g0.fa", "--kmer-guard", "--vcf", "g0.vcf"], tmp_path)
    p = run(argv + ["-o", "g1.fa", "--kmer-guard", "--vcf", "g1.vcf", "--kmer-bridge", "g.tsv"], tmp_path)
    check_pair(path("g0.fa"), path("g1.fa"), path("g.tsv"), k, R, p.stdout, "g.tsv")
    assert open(path("g1.vcf"), "rb").read() == open(path("g0.vcf"), "rb").read()
    # under a least count the reads are asked through R_2
    keys, counts = mc.read_counts([reads], k)
    R2 = mc.reliable_set(keys, counts, 2)
    p = run(argv + ["-o", "m.fa", "--qv-min-count", "2", "--kmer-bridge", "m.tsv"], tmp_path)
    check_pair(path("base.fa"), path("m.fa"), path("m.tsv"), k, R2, p.stdout, "m.tsv")
    assert no_tmp()
    # stage 0 (the reads parsed once, for the solid k-mers and the set), then stage 1 over the set that run stored: the same files
    drop_aux(tmp_path)
    p = run(argv + ["-o", "s0.fa", "--kmer-bridge", "s0.tsv"], tmp_path)
    assert "Beginning from stage: 0" in p.stdout
    p0 = run(argv + ["-o", "s0base.fa"], tmp_path)
    assert "Beginning from stage: 1" in p0.stdout
    check_pair(path("s0base.fa"), path("s0.fa"), path("s0.tsv"), k, R)
    p = run(argv + ["-o", "s1.fa", "--kmer-bridge", "s1.tsv"], tmp_path)
    assert "Beginning from stage: 1" in p.stdout
    assert open(path("s1.tsv")).read() == open(path("s0.tsv")).read() and open(path("s1.fa"), "rb").read() == open(path("s0.fa"), "rb").read()
    assert no_tmp()
