"""`hypo --kmer-fix` on the command line, without a GPU: the usage names the flag, the flag needs an argument, --qv-min-count takes it
as one of the flags it needs, and a device library without hypo_gpu_kset_query_fixes (the CPU stand-in of tests/shim) ends the run
before any stage with an error that names the entry point and the flag, leaving no output and no .tmp behind, alone and next to
--qv, --vcf, --kmer-guard and --qv-bed."""
import os
import shlex
import subprocess

import pytest

import e2e_util as eu


@pytest.fixture(scope="module")
def hypo_bin():
    try:
        return eu.build_binary()
    except Exception as e:
        pytest.skip(f"cannot build the hypo binary here: {e}")


def test_usage_names_the_flag(hypo_bin, tmp_path):
    p = subprocess.run([hypo_bin, "-h"], cwd=str(tmp_path), capture_output=True, text=True, timeout=60)
    assert p.returncode == 0
    i = p.stdout.index("--kmer-fix <str>\n")
    what = p.stdout[i:i + 1400]
    assert "[MI355X build]" in what[:60] and "[Default] no fixes." in what
    for word in ("substitution", "deletion", "insertion", "2k - 1", "--kmer-guard", "--qv-k", "--qv-min-count", "--vcf", "pos", "missing k-mers"):
        assert word in what, word
    assert i > p.stdout.index("--qv-min-count <int|valley>")


def test_flag_needs_an_argument(hypo_bin, tmp_path):
    p = subprocess.run([hypo_bin, "-c", "30", "--kmer-fix"], cwd=str(tmp_path), capture_output=True, text=True, timeout=60)
    assert "requires an argument" in p.stderr and "kmer-fix" in p.stderr
    assert "Usage: hypo <args>" in p.stdout
    assert not [f for f in os.listdir(str(tmp_path)) if f != "aux"]


def test_min_count_accepts_the_flag(hypo_bin, tmp_path):
    for argv in (["--qv-min-count", "2", "--kmer-fix", "f.tsv"], ["--kmer-fix", "f.tsv", "--qv-min-count", "valley"]):
        p = subprocess.run([hypo_bin] + argv, cwd=str(tmp_path), capture_output=True, text=True, timeout=60)
        assert "--qv-min-count" not in p.stderr and "Too few arguments" in p.stderr
    p = subprocess.run([hypo_bin, "--qv-min-count", "2"], cwd=str(tmp_path), capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and "Arg Error" in p.stderr and "--kmer-fix" in p.stderr
    assert not [f for f in os.listdir(str(tmp_path)) if f != "aux"]


@pytest.mark.parametrize("extra", [[], ["--qv", "out.qv"], ["--vcf", "out.vcf"], ["--kmer-guard"], ["--qv-bed", "out.bed"],
                                   ["--qv", "out.qv", "--vcf", "out.vcf", "--kmer-guard", "--qv-bed", "out.bed"]])
def test_fix_needs_the_entry_point(hypo_bin, tmp_path, extra):
    eu.build_shim()
    man = eu.make_inputs("e2e_20k_s1", tmp_path)
    argv = shlex.split(man["command"])
    argv[0] = hypo_bin
    argv += ["-o", "out.fa"]
    env = dict(os.environ, LD_LIBRARY_PATH=eu.SHIM_DIR + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
    p = subprocess.run(argv + ["--kmer-fix", "out.fix.tsv"] + extra, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode != 0
    assert "hypo_gpu_kset_query_fixes" in p.stderr and "--kmer-fix" in p.stderr
    assert "BATCH-ID" not in p.stdout and "Solid kmers" not in p.stdout            # before any stage
    left = sorted(os.listdir(str(tmp_path)))
    assert not [f for f in left if f.startswith("out.") or f.endswith(".tmp")], left
