"""`hypo --kmer-guard` on the command line, without a GPU: the usage names the flag, a --qv-k outside 12..31 is refused with the
guard as without it, and a device library without hypo_gpu_kset_query_spans (the CPU stand-in of tests/shim) ends the run before
any stage with an error that names the entry point, leaving no output and no .tmp behind."""
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
    i = p.stdout.index("--kmer-guard\n")
    what = p.stdout[i:i + 700]
    assert "[MI355X build]" in what[:60] and "cluster" in what and "FILTER kmer" in what and "--qv-k" in what and "[Default] off." in what
    assert i > p.stdout.index("--qv-mem <GiB>")


@pytest.mark.parametrize("k", ["11", "32", "x"])
def test_bad_qv_k_with_the_guard(hypo_bin, tmp_path, k):
    for argv in (["--kmer-guard", "--qv-k", k], ["--qv-k", k, "--kmer-guard"]):
        p = subprocess.run([hypo_bin] + argv, cwd=str(tmp_path), capture_output=True, text=True, timeout=60)
        assert p.returncode == 1
        assert "--qv-k" in p.stderr and "12" in p.stderr and "31" in p.stderr
        assert not os.listdir(str(tmp_path))


def test_flag_takes_no_argument(hypo_bin, tmp_path):
    p = subprocess.run([hypo_bin, "--kmer-guard", "--qv-k", "22"], cwd=str(tmp_path), capture_output=True, text=True, timeout=60)
    assert "Too few arguments" in p.stderr and "kmer-guard" not in p.stderr


@pytest.mark.parametrize("extra", [[], ["--vcf", "out.vcf"], ["--qv", "out.qv", "--vcf", "out.vcf"]])
def test_guard_needs_the_entry_point(hypo_bin, tmp_path, extra):
    eu.build_shim()
    man = eu.make_inputs("e2e_20k_s1", tmp_path)
    argv = shlex.split(man["command"])
    argv[0] = hypo_bin
    argv += ["-o", "out.fa"]
    env = dict(os.environ, LD_LIBRARY_PATH=eu.SHIM_DIR + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
    p = subprocess.run(argv + ["--kmer-guard"] + extra, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode != 0
    assert "hypo_gpu_kset_query_spans" in p.stderr and "--kmer-guard" in p.stderr
    assert "BATCH-ID" not in p.stdout and "Solid kmers" not in p.stdout            # before any stage
    left = sorted(os.listdir(str(tmp_path)))
    assert not [f for f in left if f.startswith("out.") or f.endswith(".tmp")], left
