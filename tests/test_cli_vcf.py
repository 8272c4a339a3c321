"""`hypo --vcf` on the command line, without a GPU: the usage lists it, a missing argument prints the usage, and a device library
without hypo_gpu_edit_scripts (the CPU stand-in of tests/shim) ends the run before any stage, leaving no output behind."""
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


def test_usage_lists_vcf(hypo_bin, tmp_path):
    p = subprocess.run([hypo_bin, "-h"], cwd=str(tmp_path), capture_output=True, text=True, timeout=60)
    assert p.returncode == 0
    i = p.stdout.index("--vcf <str>")
    assert "[MI355X build]" in p.stdout[i:i + 400] and "VCF" in p.stdout[i:i + 400]


def test_vcf_without_argument_prints_usage(hypo_bin, tmp_path):
    for argv in (["--vcf"], ["-t", "2", "--vcf"]):
        p = subprocess.run([hypo_bin] + argv, cwd=str(tmp_path), capture_output=True, text=True, timeout=60)
        q = subprocess.run([hypo_bin, "--threads"], cwd=str(tmp_path), capture_output=True, text=True, timeout=60)
        assert p.returncode == q.returncode == 0
        assert "--reads-short" in p.stdout and "requires an argument" in p.stderr and p.stdout == q.stdout


def test_vcf_needs_the_entry_point(hypo_bin, tmp_path):
    eu.build_shim()
    man = eu.make_inputs("e2e_20k_s1", tmp_path)
    argv = shlex.split(man["command"])
    argv[0] = hypo_bin
    argv += ["-o", "out.fa", "--vcf", "out.vcf"]
    env = dict(os.environ, LD_LIBRARY_PATH=eu.SHIM_DIR + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
    p = subprocess.run(argv, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode != 0
    assert "hypo_gpu_edit_scripts" in p.stderr and "--vcf" in p.stderr
    assert "BATCH-ID" not in p.stdout and "Solid kmers" not in p.stdout            # before any stage
    left = sorted(os.listdir(str(tmp_path)))
    assert not [f for f in left if f.startswith("out.")], left
    # the same run without --vcf works over the same library
    argv = argv[:-2]
    p = subprocess.run(argv, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    assert os.path.exists(str(tmp_path / "out.fa")) and not os.path.exists(str(tmp_path / "out.vcf"))
