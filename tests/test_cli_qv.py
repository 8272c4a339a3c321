"""`hypo --qv` on the command line, without a GPU: the usage lists the three flags, a missing argument prints the usage, a k-mer
length outside 12..31 is refused, and a device library without the hypo_gpu_kset_* entry points (the CPU stand-in of tests/shim)
ends the run before any stage, leaving no output behind."""
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


def test_usage_lists_the_flags(hypo_bin, tmp_path):
    p = subprocess.run([hypo_bin, "-h"], cwd=str(tmp_path), capture_output=True, text=True, timeout=60)
    assert p.returncode == 0
    for flag, word in (("--qv <str>", "QV"), ("--qv-k <int>", "12 to 31"), ("--qv-mem <GiB>", "table")):
        i = p.stdout.index(flag)
        assert "[MI355X build]" in p.stdout[i:i + 200] and word in p.stdout[i:i + 700], flag
    i = p.stdout.index("--qv <str>")
    assert "stage 1" in p.stdout[i:i + 700] and "for the QV alone" in p.stdout[i:i + 700]


def test_qv_without_argument_prints_usage(hypo_bin, tmp_path):
    q = subprocess.run([hypo_bin, "--threads"], cwd=str(tmp_path), capture_output=True, text=True, timeout=60)
    for argv in (["--qv"], ["-t", "2", "--qv"], ["--qv-k"], ["--qv-mem"]):
        p = subprocess.run([hypo_bin] + argv, cwd=str(tmp_path), capture_output=True, text=True, timeout=60)
        assert p.returncode == q.returncode == 0
        assert "--reads-short" in p.stdout and "requires an argument" in p.stderr and p.stdout == q.stdout


@pytest.mark.parametrize("k", ["11", "32", "0", "x"])
def test_qv_k_out_of_range(hypo_bin, tmp_path, k):
    p = subprocess.run([hypo_bin, "--qv", "out.qv", "--qv-k", k], cwd=str(tmp_path), capture_output=True, text=True, timeout=60)
    assert p.returncode == 1
    assert "--qv-k" in p.stderr and "12" in p.stderr and "31" in p.stderr
    assert not os.listdir(str(tmp_path))


@pytest.mark.parametrize("k", ["12", "22", "31"])
def test_qv_k_in_range_is_accepted(hypo_bin, tmp_path, k):
    p = subprocess.run([hypo_bin, "--qv", "out.qv", "--qv-k", k], cwd=str(tmp_path), capture_output=True, text=True, timeout=60)
    assert "--qv-k" not in p.stderr and "Too few arguments" in p.stderr


def test_qv_needs_the_entry_points(hypo_bin, tmp_path):
    eu.build_shim()
    man = eu.make_inputs("e2e_20k_s1", tmp_path)
    argv = shlex.split(man["command"])
    argv[0] = hypo_bin
    argv += ["-o", "out.fa", "--qv", "out.qv"]
    env = dict(os.environ, LD_LIBRARY_PATH=eu.SHIM_DIR + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
    p = subprocess.run(argv, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode != 0
    assert "hypo_gpu_kset_" in p.stderr and "--qv" in p.stderr
    assert "BATCH-ID" not in p.stdout and "Solid kmers" not in p.stdout            # before any stage
    left = sorted(os.listdir(str(tmp_path)))
    assert not [f for f in left if f.startswith("out.")], left
    # the same run without --qv works over the same library
    argv = argv[:-2]
    p = subprocess.run(argv, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    assert os.path.exists(str(tmp_path / "out.fa")) and not os.path.exists(str(tmp_path / "out.qv"))
    assert "QV" not in p.stdout
