"""GPU: `hypo --kmer-fix` end to end.  The golden sets as they stand have next to nothing to fix, so the scenario leaves the polish
without alignments on the second half of every contig: the SAM files keep their header lines and the records whose POS is below
half their contig's LN, the reads file stays whole.  The k-mers of the reads then pin down the draft errors the polish could not
reach.  For every set the run without the flag gives the base FASTA and stdout; with the flag the FASTA is the checker's
(tests/kmer_fix_checker.py) over the base FASTA, the TSV is the checker's text and applied backwards turns the base FASTA into the
new one, stdout differs by the one Info line, whose numbers are the checker's, and no .tmp is left.  Then next to the other flags."""
import os
import re

import pytest

import e2e_util as eu
import edit_checker as ec
import kmer_fix_checker as fc
import min_count_checker as mc
import qv_checker as qc
import qv_track_checker as tc
from test_gpu_qv import drop_aux, golden_argv, opt, run
from test_gpu_qv_bed import stable

pytestmark = pytest.mark.gpu
INFO = r"^\[Hypo::Hypo\] Info: k-mer fix .*$"


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(eu.BIN):
        eu.build_binary()


def cut_sams(tmp_path):
    """the header lines, and the records whose POS is below half their contig's LN"""
    cut = 0
    for f in ("sr.sam", "lr.sam"):
        p = os.path.join(str(tmp_path), f)
        if not os.path.exists(p):
            continue
        ln, keep = {}, []
        for line in open(p):
            if line.startswith("@"):
                if line.startswith("@SQ"):
                    tags = dict(t.split(":", 1) for t in line.rstrip("\n").split("\t")[1:])
                    ln[tags["SN"]] = int(tags["LN"])
                keep.append(line)
                continue
            fld = line.split("\t", 4)
            if 2 * int(fld[3]) < ln[fld[2]]:
                keep.append(line)
            else:
                cut += 1
        open(p, "w").writelines(keep)
    assert cut > 0
    return cut


def scenario(name, tmp_path):
    man, argv = golden_argv(name, tmp_path)
    cut_sams(tmp_path)
    base_name = os.path.basename(opt(argv, "-d"))
    out = opt(argv, "-o", "hypo_" + (base_name[:base_name.rfind(".")] if "." in base_name else base_name) + ".fasta")
    return argv, os.path.join(str(tmp_path), out), os.path.join(str(tmp_path), opt(argv, "-r"))


def fasta_bytes(contigs):
    return "".join(f">{n}\n{s}\n" for n, s in contigs).encode()


def apply_backwards(contigs, rows):
    out = []
    for name, s in contigs:
        b = bytearray(s.encode())
        for _, pos, kind, ref, alt, _ in reversed([r for r in rows if r[0] == name]):
            if kind != "ins":
                assert b[pos:pos + 1] == ref.encode()
            b[pos:pos + (kind != "ins")] = b"" if kind == "del" else alt.encode()
        out.append((name, b.decode()))
    return out


def check_pair(base_fa, fixed_fa, tsv_path, k, R, stdout=None, tsv_name=None):
    """the fixed FASTA and the TSV against the checker run on the base FASTA; returns (rows of the TSV, the checker's stats)"""
    base = ec.read_fastx(base_fa)
    want, want_tsv, st = fc.run(base, k, R)
    got = open(fixed_fa, "rb").read()
    assert got == fasta_bytes(want), "the FASTA is not the checker's"
    text = open(tsv_path).read()
    assert text == want_tsv
    rows = fc.parse_tsv(text)
    assert fasta_bytes(apply_backwards(base, rows)) == got
    assert [r[0] for r in rows] == sorted((r[0] for r in rows), key=[n for n, _ in base].index)          # contigs in draft order
    if stdout is not None:
        info = re.findall(INFO, stdout, flags=re.M)
        assert info == [fc.info_line(tsv_name, k, st)], (info, fc.info_line(tsv_name, k, st))
    return rows, st


@pytest.mark.parametrize("name,k", [("e2e_20k_s1", None), ("e2e_20k_s1", 31), ("e2e_5ctg_long_s21", None)])
def test_fix_pair(name, k, tmp_path):
    argv, out_path, reads = scenario(name, tmp_path)
    if name == "e2e_5ctg_long_s21":
        assert opt(argv, "-p") == "2" and "-B" in argv
    kk = 21 if k is None else k
    kargs = [] if k is None else ["--qv-k", str(k)]
    R = qc.read_set([reads], kk)
    no_tmp = lambda: not [f for f in os.listdir(str(tmp_path)) if f.endswith(".tmp")]
    p0 = run(argv, tmp_path)
    assert "k-mer fix" not in p0.stdout
    base_fa = str(tmp_path / "base.fa")
    os.rename(out_path, base_fa)
    p = run(argv + ["--kmer-fix", "f.tsv"] + kargs, tmp_path)
    rows, st = check_pair(base_fa, out_path, str(tmp_path / "f.tsv"), kk, R, p.stdout, "f.tsv")
    assert stable(p.stdout, ["[Hypo::Hypo] Info: k-mer fix "]) == stable(p0.stdout)
    assert len(stable(p.stdout)) == len(stable(p0.stdout)) + 1
    assert no_tmp()
    kinds = [r[2] for r in rows]
    if name == "e2e_20k_s1":
        assert len(rows) >= 10 and all(kinds.count(x) >= 1 for x in ("sub", "del", "ins")), kinds
    else:
        first = ec.read_fastx(base_fa)[0][0]
        assert sum(1 for r in rows if r[0] == first) >= 10
    assert st.fixed == len(rows) and st.removed == sum(r[5] for r in rows)


@pytest.mark.parametrize("name", ["e2e_20k_s1", "e2e_5ctg_long_s21"])
def test_fix_with_the_other_flags(name, tmp_path):
    """the multi-contig set: what is per contig (--vcf, --qv, --qv-bed, -p 1); the small set: the guard, the least count and the
    stages as well"""
    argv, out_path, reads = scenario(name, tmp_path)
    k = 21
    R = qc.read_set([reads], k)
    path = lambda f: str(tmp_path / f)
    no_tmp = lambda: not [f for f in os.listdir(str(tmp_path)) if f.endswith(".tmp")]
    # --vcf and --qv without and with the flag: the same VCF bytes; polished_missing drops per contig by the sum of missing_kmers
    run(argv + ["-o", "base.fa", "--vcf", "v0.vcf", "--qv", "q0.tsv"], tmp_path)
    p = run(argv + ["-o", "fixed.fa", "--vcf", "v1.vcf", "--qv", "q1.tsv", "--qv-bed", "b.bed", "--kmer-fix", "f.tsv"], tmp_path)
    rows, st = check_pair(path("base.fa"), path("fixed.fa"), path("f.tsv"), k, R, p.stdout, "f.tsv")
    assert rows
    assert open(path("v1.vcf"), "rb").read() == open(path("v0.vcf"), "rb").read()
    t0, t1 = qc.parse_table(open(path("q0.tsv")).read()), qc.parse_table(open(path("q1.tsv")).read())
    removed = {}
    for r in rows:
        removed[r[0]] = removed.get(r[0], 0) + r[5]
    removed["*"] = sum(removed.values())
    assert [(a[0], a[1], a[2], a[3]) for a in t0] == [(b[0], b[1], b[2], b[3]) for b in t1]              # the draft columns do not move
    assert [(a[0], a[4] - b[4]) for a, b in zip(t0, t1)] == [(a[0], removed.get(a[0], 0)) for a in t0]
    fixed = ec.read_fastx(path("fixed.fa"))
    assert [(r[0], r[4], r[5]) for r in t1[:-1]] == [(n, m, t) for n, (t, m) in ((n, qc.seq_stats(s, k, R)) for n, s in fixed)]
    assert open(path("b.bed")).read() == tc.bed(fixed, k, R)
    assert no_tmp()
    tsv, fixed_bytes = open(path("f.tsv")).read(), open(path("fixed.fa"), "rb").read()
    # -p 1 writes the same files
    a1 = list(argv)
    if "-p" in a1:
        a1[a1.index("-p") + 1] = "1"
    else:
        a1 += ["-p", "1"]
    run(a1 + ["-o", "p1.fa", "--kmer-fix", "p1.tsv"], tmp_path)
    assert open(path("p1.tsv")).read() == tsv and open(path("p1.fa"), "rb").read() == fixed_bytes
    if name != "e2e_20k_s1":
        return
    # with the guard: the fixes are made over the guarded text, and the VCF is the guard's
    run(argv + ["-o", "g0.fa", "--kmer-guard", "--vcf", "g0.vcf"], tmp_path)
    p = run(argv + ["-o", "g1.fa", "--kmer-guard", "--vcf", "g1.vcf", "--kmer-fix", "g.tsv"], tmp_path)
    check_pair(path("g0.fa"), path("g1.fa"), path("g.tsv"), k, R, p.stdout, "g.tsv")
    assert open(path("g1.vcf"), "rb").read() == open(path("g0.vcf"), "rb").read()
    # under a least count the reads are asked through R_2
    keys, counts = mc.read_counts([reads], k)
    R2 = mc.reliable_set(keys, counts, 2)
    p = run(argv + ["-o", "m.fa", "--qv-min-count", "2", "--kmer-fix", "m.tsv"], tmp_path)
    check_pair(path("base.fa"), path("m.fa"), path("m.tsv"), k, R2, p.stdout, "m.tsv")
    assert no_tmp()
    # stage 0 (the reads parsed once, for the solid k-mers and the set), then stage 1 over the set that run stored: the same files
    drop_aux(tmp_path)
    p = run(argv + ["-o", "s0.fa", "--kmer-fix", "s0.tsv"], tmp_path)
    assert "Beginning from stage: 0" in p.stdout
    p0 = run(argv + ["-o", "s0base.fa"], tmp_path)
    assert "Beginning from stage: 1" in p0.stdout
    check_pair(path("s0base.fa"), path("s0.fa"), path("s0.tsv"), k, R)
    p = run(argv + ["-o", "s1.fa", "--kmer-fix", "s1.tsv"], tmp_path)
    assert "Beginning from stage: 1" in p.stdout
    assert open(path("s1.tsv")).read() == open(path("s0.tsv")).read() and open(path("s1.fa"), "rb").read() == open(path("s0.fa"), "rb").read()
    assert no_tmp()
