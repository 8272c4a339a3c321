"""`hypo --qv-spectra` on the command line, without a GPU: the usage names both flags, they need an argument, --qv-reliable-min is
range-checked before anything is created, and a device library without the three entry points (the CPU stand-in of tests/shim)
ends the run before any stage with an error that names them and the flag, leaving no output and no .tmp behind, while the same
run without the flag works."""
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
    i = p.stdout.index("--qv-spectra <str>\n")
    what = p.stdout[i:i + 1300]
    assert "[MI355X build]" in what[:60] and "copy-number spectrum" in what and "completeness" in what and "--qv-k" in what and "[Default] no spectra." in what
    j = p.stdout.index("--qv-reliable-min <int>\n")
    what = p.stdout[j:j + 400]
    assert "[MI355X build]" in what[:60] and "1 to 255" in what and "valley" in what
    assert j > i > p.stdout.index("--qv-bed <str>")


def test_flags_need_an_argument(hypo_bin, tmp_path):
    q = subprocess.run([hypo_bin, "--threads"], cwd=str(tmp_path), capture_output=True, text=True, timeout=60)
    for argv in (["--qv-spectra"], ["-c", "30", "--qv-spectra"], ["--qv-reliable-min"]):
        p = subprocess.run([hypo_bin] + argv, cwd=str(tmp_path), capture_output=True, text=True, timeout=60)
        assert p.returncode == q.returncode == 0
        assert "requires an argument" in p.stderr and "Usage: hypo <args>" in p.stdout and p.stdout == q.stdout
    assert not [f for f in os.listdir(str(tmp_path)) if f != "aux"]


@pytest.mark.parametrize("v", ["0", "256", "x", "-3", "7x", ""])
def test_reliable_min_out_of_range(hypo_bin, tmp_path, v):
    p = subprocess.run([hypo_bin, "--qv-spectra", "out.tsv", "--qv-reliable-min", v], cwd=str(tmp_path), capture_output=True, text=True, timeout=60)
    assert p.returncode == 1
    assert "--qv-reliable-min" in p.stderr and "1" in p.stderr and "255" in p.stderr
    assert not os.listdir(str(tmp_path))


@pytest.mark.parametrize("v", ["1", "7", "255"])
def test_reliable_min_in_range_is_accepted(hypo_bin, tmp_path, v):
    p = subprocess.run([hypo_bin, "--qv-spectra", "out.tsv", "--qv-reliable-min", v], cwd=str(tmp_path), capture_output=True, text=True, timeout=60)
    assert "--qv-reliable-min" not in p.stderr and "Too few arguments" in p.stderr


@pytest.mark.parametrize("extra", [[], ["--qv-reliable-min", "3"], ["--qv", "out.qv", "--qv-bed", "out.bed", "--vcf", "out.vcf", "--kmer-guard"]])
def test_spectra_need_the_entry_points(hypo_bin, tmp_path, extra):
    eu.build_shim()
    man = eu.make_inputs("e2e_20k_s1", tmp_path)
    argv = shlex.split(man["command"])
    argv[0] = hypo_bin
    argv += ["-o", "out.fa"]
    env = dict(os.environ, LD_LIBRARY_PATH=eu.SHIM_DIR + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
    p = subprocess.run(argv + ["--qv-spectra", "out.tsv"] + extra, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode != 0
    for name in ("hypo_gpu_kset_counts_enable", "hypo_gpu_kset_mark", "hypo_gpu_kset_spectrum", "--qv-spectra"):
        assert name in p.stderr, p.stderr
    assert "BATCH-ID" not in p.stdout and "Solid kmers" not in p.stdout            # before any stage
    left = sorted(os.listdir(str(tmp_path)))
    assert not [f for f in left if f.startswith("out.") or f.endswith(".tmp")], left
    if not extra:
        # the same run without the flag works over the stand-in
        q = subprocess.run(argv, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
        assert q.returncode == 0, q.stdout[-1500:] + q.stderr[-1500:]
        assert os.path.exists(str(tmp_path / "out.fa")) and not os.path.exists(str(tmp_path / "out.tsv"))
        assert "spectra" not in q.stdout
        assert not [f for f in os.listdir(str(tmp_path)) if f.endswith(".tmp")]
