"""`hypo --qv-min-count` on the command line, without a GPU: the usage names the flag, it needs an argument, its value is checked
and a run without anything that asks the reads is refused before anything is created, and a device library without the three entry
points (the CPU stand-in of tests/shim) ends the run before any stage with an error that names them and the flag, leaving no output
and no .tmp behind, while `--qv-min-count 1`, the run without the flag, works over it."""
import os
import shlex
import subprocess

import pytest

import e2e_util as eu

CONSUMERS = (["--qv", "out.qv"], ["--qv-bed", "out.bed"], ["--kmer-guard"], ["--guard-records"])


@pytest.fixture(scope="module")
def hypo_bin():
    try:
        return eu.build_binary()
    except Exception as e:
        pytest.skip(f"cannot build the hypo binary here: {e}")


def run(hypo_bin, tmp_path, argv, **kw):
    return subprocess.run([hypo_bin] + argv, cwd=str(tmp_path), capture_output=True, text=True, timeout=kw.pop("timeout", 60), **kw)


def test_usage_lists_the_flag(hypo_bin, tmp_path):
    p = run(hypo_bin, tmp_path, ["-h"])
    assert p.returncode == 0
    i = p.stdout.index("--qv-min-count <int|valley>\n")
    what = p.stdout[i:i + 1200]
    assert "[MI355X build]" in what[:70] and "1 to 255" in what and "valley" in what and "[Default] 1: a k-mer seen once is present." in what
    for flag in ("--qv", "--qv-bed", "--kmer-guard", "--guard-records", "--qv-reliable-min", "--qv-spectra", "--qv-mem"):
        assert flag in what, flag
    assert i > p.stdout.index("--qv-reliable-min <int>")


def test_flag_needs_an_argument(hypo_bin, tmp_path):
    q = run(hypo_bin, tmp_path, ["--threads"])
    for argv in (["--qv-min-count"], ["--qv", "out.qv", "--qv-min-count"]):
        p = run(hypo_bin, tmp_path, argv)
        assert p.returncode == q.returncode == 0
        assert "requires an argument" in p.stderr and "Usage: hypo <args>" in p.stdout and p.stdout == q.stdout
    assert not [f for f in os.listdir(str(tmp_path)) if f != "aux"]


@pytest.mark.parametrize("v", ["0", "256", "x", "7x", "", "-3", "Valley", "valleys"])
def test_value_out_of_range(hypo_bin, tmp_path, v):
    p = run(hypo_bin, tmp_path, ["--qv", "out.qv", "--qv-min-count", v])
    assert p.returncode == 1
    assert "Arg Error" in p.stderr and "--qv-min-count" in p.stderr and "1" in p.stderr and "255" in p.stderr and "valley" in p.stderr
    assert not os.listdir(str(tmp_path))


@pytest.mark.parametrize("v", ["1", "7", "255", "valley"])
@pytest.mark.parametrize("consumer", CONSUMERS, ids=lambda c: c[0])
def test_value_in_range_is_accepted(hypo_bin, tmp_path, v, consumer):
    for argv in (consumer + ["--qv-min-count", v], ["--qv-min-count", v] + consumer):
        p = run(hypo_bin, tmp_path, argv)
        assert "--qv-min-count" not in p.stderr and "Too few arguments" in p.stderr


@pytest.mark.parametrize("v", ["2", "255", "valley"])
def test_flag_without_a_consumer(hypo_bin, tmp_path, v):
    """nothing that asks the reads: neither a complete command line nor --qv-spectra, --vcf or --qv-k make it one"""
    man = eu.make_inputs("e2e_20k_s1", tmp_path)
    before = sorted(os.listdir(str(tmp_path)))
    full = shlex.split(man["command"])[1:]
    for argv in ([], ["--qv-spectra", "out.tsv", "--vcf", "out.vcf", "--qv-k", "16"], full, full + ["--qv-spectra", "out.tsv"]):
        p = run(hypo_bin, tmp_path, argv + ["--qv-min-count", v])
        assert p.returncode == 1
        assert "Arg Error" in p.stderr and "--qv-min-count" in p.stderr
        for flag in ("--qv", "--qv-bed", "--kmer-guard", "--guard-records"):
            assert flag in p.stderr
        assert "Beginning from stage" not in p.stdout
    assert sorted(os.listdir(str(tmp_path))) == before                     # not even aux/
    # 1 is the run without the flag: it asks for nothing
    p = run(hypo_bin, tmp_path, ["--qv-min-count", "1"])
    assert "--qv-min-count" not in p.stderr and "Too few arguments" in p.stderr


@pytest.mark.parametrize("extra", [["--qv", "out.qv", "--qv-min-count", "2"], ["--kmer-guard", "--qv-min-count", "valley"],
                                   ["--qv-min-count", "3", "--qv-spectra", "out.tsv", "--qv", "out.qv", "--qv-bed", "out.bed", "--vcf", "out.vcf", "--guard-records"]],
                         ids=["qv", "guard", "everything"])
def test_min_count_needs_the_entry_points(hypo_bin, tmp_path, extra):
    eu.build_shim()
    man = eu.make_inputs("e2e_20k_s1", tmp_path)
    argv = shlex.split(man["command"])[1:] + ["-o", "out.fa"]
    env = dict(os.environ, LD_LIBRARY_PATH=eu.SHIM_DIR + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
    p = run(hypo_bin, tmp_path, argv + extra, env=env, timeout=300)
    assert p.returncode != 0
    for name in ("hypo_gpu_kset_counts_enable", "hypo_gpu_kset_spectrum", "hypo_gpu_kset_min_count", "--qv-min-count"):
        assert name in p.stderr, p.stderr
    assert "BATCH-ID" not in p.stdout and "Solid kmers" not in p.stdout            # before any stage
    left = sorted(os.listdir(str(tmp_path)))
    assert not [f for f in left if f.startswith("out.") or f.endswith(".tmp")], left
    if extra[0] == "--qv":
        # --qv-min-count 1 is the run without the flag: over the stand-in it works, and looks up none of the three
        q = run(hypo_bin, tmp_path, argv + ["--qv-min-count", "1"], env=env, timeout=600)
        assert q.returncode == 0, q.stdout[-1500:] + q.stderr[-1500:]
        assert os.path.exists(str(tmp_path / "out.fa")) and "min count" not in q.stdout and "hypo_gpu_kset" not in q.stderr
        assert not [f for f in os.listdir(str(tmp_path)) if f.endswith(".tmp")]
        # ... while with something that asks the reads it is that flag's entry points the stand-in lacks, not these
        r = run(hypo_bin, tmp_path, argv + ["--qv", "out.qv", "--qv-min-count", "1"], env=env, timeout=300)
        assert r.returncode != 0 and "--qv needs" in r.stderr and "hypo_gpu_kset_min_count" not in r.stderr and "--qv-min-count" not in r.stderr
