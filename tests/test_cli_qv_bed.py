"""`hypo --qv-bed` on the command line, without a GPU: the usage names the flag, the flag needs an argument, and a device library
without hypo_gpu_kset_query_track (the CPU stand-in of tests/shim) ends the run before any stage with an error that names the entry
point and the flag, leaving no output and no .tmp behind, alone and next to --qv, --vcf and --kmer-guard."""
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
    i = p.stdout.index("--qv-bed <str>\n")
    what = p.stdout[i:i + 900]
    assert "[MI355X build]" in what[:60] and "BED" in what and "polished_missing" in what and "--qv-k" in what and "[Default] no BED." in what
    assert i > p.stdout.index("--guard-records-max <int>")


def test_flag_needs_an_argument(hypo_bin, tmp_path):
    p = subprocess.run([hypo_bin, "-c", "30", "--qv-bed"], cwd=str(tmp_path), capture_output=True, text=True, timeout=60)
    assert "requires an argument" in p.stderr and "qv-bed" in p.stderr
    assert "Usage: hypo <args>" in p.stdout
    assert not [f for f in os.listdir(str(tmp_path)) if f != "aux"]


@pytest.mark.parametrize("extra", [[], ["--qv", "out.qv"], ["--vcf", "out.vcf"], ["--kmer-guard"], ["--qv", "out.qv", "--vcf", "out.vcf", "--kmer-guard"]])
def test_track_needs_the_entry_point(hypo_bin, tmp_path, extra):
    eu.build_shim()
    man = eu.make_inputs("e2e_20k_s1", tmp_path)
    argv = shlex.split(man["command"])
    argv[0] = hypo_bin
    argv += ["-o", "out.fa"]
    env = dict(os.environ, LD_LIBRARY_PATH=eu.SHIM_DIR + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
    p = subprocess.run(argv + ["--qv-bed", "out.bed"] + extra, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode != 0
    assert "hypo_gpu_kset_query_track" in p.stderr and "--qv-bed" in p.stderr
    assert "BATCH-ID" not in p.stdout and "Solid kmers" not in p.stdout            # before any stage
    left = sorted(os.listdir(str(tmp_path)))
    assert not [f for f in left if f.startswith("out.") or f.endswith(".tmp")], left
