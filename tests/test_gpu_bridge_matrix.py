"""GPU: a report flag changes neither the FASTA nor the bridge TSV.  As tests/test_gpu_extras_matrix.py, over the cut and planted
e2e_20k_s1 set (planted_scenario() of tests/test_gpu_kmer_bridge.py: bridges exist), for the sets of text-changing flags that hold
--kmer-bridge (alone, behind the fix, behind the guard and the fix): one run with all four report flags (--vcf --qv --qv-bed
--qv-spectra) and four runs with one of them each.  The FASTA, the bridge TSV, and the fixes TSV where there is one, are the same bytes
in all five runs; every report file of the run with all four is byte-equal to that of the run that asked for it alone; no .tmp is
left."""
import os

import pytest

import e2e_util as eu
from test_gpu_kmer_bridge import planted_scenario
from test_gpu_qv import run

pytestmark = pytest.mark.gpu

REPORTS = [("--vcf", "vcf"), ("--qv", "qv.tsv"), ("--qv-bed", "bed"), ("--qv-spectra", "spectra.tsv")]
TEXT_FLAGS = {
    "bridge": ["--kmer-bridge", "b.tsv"],
    "fix_bridge": ["--kmer-fix", "f.tsv", "--kmer-bridge", "b.tsv"],
    "guard_fix_bridge": ["--kmer-guard", "--kmer-fix", "f.tsv", "--kmer-bridge", "b.tsv"],
}


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(eu.BIN):
        eu.build_binary()


@pytest.mark.parametrize("t", list(TEXT_FLAGS))
def test_a_report_flag_changes_no_other_file(t, tmp_path):
    argv, _, _ = planted_scenario("e2e_20k_s1", tmp_path)
    read = lambda f: open(os.path.join(str(tmp_path), f), "rb").read()
    has_fix = "--kmer-fix" in TEXT_FLAGS[t]

    def one(tag, reports):
        """a run that writes <tag>.fa and <tag>.<ext> for every report asked for; returns (FASTA, bridge TSV, fixes TSV or None)"""
        args = argv + ["-o", tag + ".fa"] + TEXT_FLAGS[t]
        for flag, ext in reports:
            args += [flag, tag + "." + ext]
        run(args, tmp_path)
        return read(tag + ".fa"), read("b.tsv"), read("f.tsv") if has_fix else None

    fasta, bridges, fixes = one("all", REPORTS)
    assert fasta.count(b">") == 1 and len(fasta) > 19000                  # (a 20 kbp contig; the bridges take a few bases more out than they put in)
    assert bridges.count(b"\n") > 10, "the scenario has nothing to bridge"
    assert not has_fix or fixes.count(b"\n") > 1, "the scenario has nothing to fix"
    for flag, ext in REPORTS:
        tag = "only_" + ext.split(".")[0]
        fa, br, fx = one(tag, [(flag, ext)])
        assert fa == fasta, f"{flag} alone: another FASTA than with all four reports"
        assert br == bridges, f"{flag} alone: another bridge TSV than with all four reports"
        assert fx == fixes, f"{flag} alone: another fixes TSV than with all four reports"
        assert read(tag + "." + ext) == read("all." + ext), f"{flag}: its file differs between the run alone and the run with all four reports"
        assert len(read("all." + ext)) > 0
    assert not [f for f in os.listdir(str(tmp_path)) if f.endswith(".tmp")]
