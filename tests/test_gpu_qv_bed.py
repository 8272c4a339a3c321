"""GPU: `hypo --qv-bed` end to end.  For every set: the FASTA is the one the run without the flag writes (and the golden's), stdout
differs only by the QV track Info line and timings, no .tmp is left, the BED is the checker's (tests/qv_track_checker.py) computed
from the run's own reads and output FASTA, with --qv the fourth column adds up per contig to polished_missing and the table is the
one --qv alone writes, with --kmer-guard the BED describes the guarded FASTA, and -p 1 and a run from stage 1 write the same file."""
import hashlib
import os
import re
import subprocess

import pytest

import e2e_util as eu
import edit_checker as ec
import qv_checker as qc
import qv_track_checker as tc
from test_gpu_qv import drop_aux, golden_argv, opt, run

pytestmark = pytest.mark.gpu
INFO = r"\[Hypo::Hypo\] Info: QV track (\S+) \(k = (\d+)\): (\d+) intervals covering (\d+) bases, (\d+) missing k-mers$"


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(eu.BIN):
        eu.build_binary()


def stable(text, drop=()):
    return sorted(l for l in text.splitlines() if not l.startswith("RESOURCES") and not any(l.startswith(d) for d in drop))


def check_bed(path, fasta_path, k, R, stdout):
    """the file against the checker's for that FASTA, and the Info line against the file"""
    text = open(path).read()
    contigs = ec.read_fastx(fasta_path)
    assert text == tc.bed(contigs, k, R)
    rows = tc.parse_bed(text)
    info = re.findall(INFO, stdout, flags=re.M)
    assert len(info) == 1, stdout[-1500:]
    assert info[0] == (os.path.basename(path), str(k), str(len(rows)), str(sum(b - a for _, a, b, _ in rows)), str(sum(r[3] for r in rows)))
    return text, rows


@pytest.mark.parametrize("name,k", [("e2e_20k_s1", None), ("e2e_200k_long_s3", None), ("e2e_5ctg_long_s21", 16)])
def test_bed_goldens(name, k, tmp_path):
    """a plain set, a -B set and a multi-contig -p 2 set; each comes with its own aux/ (the golden FASTA is the stage-1 run's)"""
    man, argv = golden_argv(name, tmp_path)
    assert "-i" in argv and os.path.exists(str(tmp_path / "aux" / "stage.txt"))
    if name == "e2e_5ctg_long_s21":
        assert opt(argv, "-p") == "2"
    if name == "e2e_200k_long_s3":
        assert "-B" in argv
    kk = 21 if k is None else k
    kargs = [] if k is None else ["--qv-k", str(k)]
    path = lambda f: str(tmp_path / f)
    base_name = os.path.basename(opt(argv, "-d"))
    out_path = path(opt(argv, "-o", "hypo_" + (base_name[:base_name.rfind(".")] if "." in base_name else base_name) + ".fasta"))
    reads = opt(argv, "-r")
    R = qc.read_set([reads if reads.startswith("@") else path(reads)], kk)
    no_tmp = lambda: not [f for f in os.listdir(str(tmp_path)) if f.endswith(".tmp")]

    # without the flag, then with it: the same FASTA (the golden's), the same stdout but for one line
    p0 = run(argv, tmp_path)
    base = open(out_path, "rb").read()
    assert hashlib.md5(base).hexdigest() == man["expected_fasta_md5"], "polished FASTA differs from the golden"
    assert "QV track" not in p0.stdout
    p = run(argv + ["--qv-bed", "a.bed"] + kargs, tmp_path)
    assert open(out_path, "rb").read() == base, "--qv-bed changed the FASTA"
    assert stable(p.stdout, ["[Hypo::Hypo] Info: QV track "]) == stable(p0.stdout)
    assert len(stable(p.stdout)) == len(stable(p0.stdout)) + 1
    bed, rows = check_bed(path("a.bed"), out_path, kk, R, p.stdout)
    assert rows, "a set without a missing k-mer checks nothing"
    assert no_tmp()

    # with --qv: the table of --qv alone, and per contig the fourth column adds up to polished_missing
    run(argv + ["--qv", "alone.tsv"] + kargs, tmp_path)
    p = run(argv + ["--qv", "both.tsv", "--qv-bed", "b.bed"] + kargs, tmp_path)
    assert open(path("both.tsv")).read() == open(path("alone.tsv")).read()
    assert open(path("b.bed")).read() == bed and open(out_path, "rb").read() == base
    assert "Info: QV both.tsv" in p.stdout and "Info: QV track b.bed" in p.stdout
    table = qc.parse_table(open(path("both.tsv")).read())
    sums = {}
    for cname, _, _, n in rows:
        sums[cname] = sums.get(cname, 0) + n
    assert [(r[0], sums.get(r[0], 0)) for r in table[:-1]] == [(r[0], r[4]) for r in table[:-1]]
    assert sum(sums.values()) == table[-1][4]

    # -p 1 writes the same file
    a1 = list(argv)
    if "-p" in a1:
        a1[a1.index("-p") + 1] = "1"
    else:
        a1 += ["-p", "1"]
    run(a1 + ["--qv-bed", "p1.bed"] + kargs, tmp_path)
    assert open(path("p1.bed")).read() == bed

    # with the guard the BED describes the guarded text (also next to --vcf)
    p = run(argv + ["-o", "guarded.fa", "--kmer-guard", "--vcf", "g.vcf", "--qv-bed", "g.bed"] + kargs, tmp_path)
    check_bed(path("g.bed"), path("guarded.fa"), kk, R, p.stdout)
    assert no_tmp()

    # stage 0 (the reads parsed once, for the solid k-mers and the set), then stage 1 over the set that run stored: the same file
    drop_aux(tmp_path)
    p = run(argv + ["--qv-bed", "s0.bed"] + kargs, tmp_path)
    assert "Beginning from stage: 0" in p.stdout
    s0, _ = check_bed(path("s0.bed"), out_path, kk, R, p.stdout)
    fasta0 = open(out_path, "rb").read()
    p = run(argv + ["--qv-bed", "s1.bed"] + kargs, tmp_path)
    assert "Beginning from stage: 1" in p.stdout and open(out_path, "rb").read() == fasta0
    assert open(path("s1.bed")).read() == s0
    assert no_tmp()
