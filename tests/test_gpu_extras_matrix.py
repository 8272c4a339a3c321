"""GPU: a report flag changes no other file.  Over the cut e2e_20k_s1 set (scenario() of tests/test_gpu_kmer_fix.py: fixes exist), for
every set T of text-changing flags (none, the guard, the fix, both, both with --guard-records): one run with all four report flags
(--vcf --qv --qv-bed --qv-spectra) and four runs with one of them each.  The FASTA, and the fixes TSV where T has one, are the same
bytes in all five runs; every report file of the run with all four is byte-equal to that of the run that asked for it alone; no .tmp is
left.  What each file holds is the business of the flags' own tests; this one pins that the writer hands every contig's texts to each
report the same way whoever else is listening."""
import os

import pytest

import e2e_util as eu
from test_gpu_kmer_fix import scenario
from test_gpu_qv import run

pytestmark = pytest.mark.gpu

REPORTS = [("--vcf", "vcf"), ("--qv", "qv.tsv"), ("--qv-bed", "bed"), ("--qv-spectra", "spectra.tsv")]
TEXT_FLAGS = {
    "none": [],
    "guard": ["--kmer-guard"],
    "fix": ["--kmer-fix", "f.tsv"],
    "guard_fix": ["--kmer-guard", "--kmer-fix", "f.tsv"],
    "guard_records_fix": ["--kmer-guard", "--guard-records", "--kmer-fix", "f.tsv"],
}


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(eu.BIN):
        eu.build_binary()


@pytest.mark.parametrize("t", list(TEXT_FLAGS))
def test_a_report_flag_changes_no_other_file(t, tmp_path):
    argv, _, _ = scenario("e2e_20k_s1", tmp_path)
    read = lambda f: open(os.path.join(str(tmp_path), f), "rb").read()
    has_fix = "--kmer-fix" in TEXT_FLAGS[t]

    def one(tag, reports):
        """a run that writes <tag>.fa and <tag>.<ext> for every report asked for; returns (FASTA, fixes TSV or None)"""
        args = argv + ["-o", tag + ".fa"] + TEXT_FLAGS[t]
        for flag, ext in reports:
            args += [flag, tag + "." + ext]
        run(args, tmp_path)
        return read(tag + ".fa"), read("f.tsv") if has_fix else None

    fasta, fixes = one("all", REPORTS)
    assert fasta.count(b">") == 1 and len(fasta) > 20000
    assert not has_fix or fixes.count(b"\n") > 1, "the scenario has nothing to fix"
    for flag, ext in REPORTS:
        tag = "only_" + ext.split(".")[0]
        fa, fx = one(tag, [(flag, ext)])
        assert fa == fasta, f"{flag} alone: another FASTA than with all four reports"
        assert fx == fixes, f"{flag} alone: another fixes TSV than with all four reports"
        assert read(tag + "." + ext) == read("all." + ext), f"{flag}: its file differs between the run alone and the run with all four reports"
        assert len(read("all." + ext)) > 0
    assert not [f for f in os.listdir(str(tmp_path)) if f.endswith(".tmp")]
