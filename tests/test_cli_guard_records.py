"""`hypo --guard-records` on the command line, without a GPU: the usage names both flags after --kmer-guard, a --guard-records-max
outside 2..12 is refused with the range, the flag takes no argument, and a device library without hypo_gpu_kset_query_variants (the
CPU stand-in of tests/shim) ends the run before any stage with an error that names the entry point, leaving no output and no .tmp."""
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


def test_usage_names_the_flags(hypo_bin, tmp_path):
    p = subprocess.run([hypo_bin, "-h"], cwd=str(tmp_path), capture_output=True, text=True, timeout=60)
    assert p.returncode == 0
    g, i, j = p.stdout.index("--kmer-guard\n"), p.stdout.index("--guard-records\n"), p.stdout.index("--guard-records-max <int>\n")
    assert g < i < j < p.stdout.index("-h, --help")
    what = p.stdout[i:j]
    assert "[MI355X build]" in what[:60] and "--kmer-guard" in what and "subset" in what and "FILTER kmer" in what and "[Default] off." in what
    what = p.stdout[j:j + 400]
    assert "[MI355X build]" in what[:60] and "2 to 12" in what and "[Default] 8." in what


@pytest.mark.parametrize("n", ["1", "13", "x", "0", "-3", "8x", ""])
def test_bad_guard_records_max(hypo_bin, tmp_path, n):
    for argv in (["--guard-records", "--guard-records-max", n], ["--guard-records-max", n]):
        p = subprocess.run([hypo_bin] + argv, cwd=str(tmp_path), capture_output=True, text=True, timeout=60)
        assert p.returncode == 1
        assert "Arg Error" in p.stderr and "--guard-records-max" in p.stderr and "2" in p.stderr and "12" in p.stderr
        assert not os.listdir(str(tmp_path))


@pytest.mark.parametrize("n", ["2", "8", "12"])
def test_good_guard_records_max(hypo_bin, tmp_path, n):
    p = subprocess.run([hypo_bin, "--guard-records-max", n], cwd=str(tmp_path), capture_output=True, text=True, timeout=60)
    assert "Too few arguments" in p.stderr and "Arg Error" not in p.stderr


def test_flag_takes_no_argument(hypo_bin, tmp_path):
    p = subprocess.run([hypo_bin, "--guard-records", "--guard-records-max", "4"], cwd=str(tmp_path), capture_output=True, text=True, timeout=60)
    assert "Too few arguments" in p.stderr and "guard-records" not in p.stderr


@pytest.mark.parametrize("extra", [[], ["--kmer-guard"], ["--guard-records-max", "4", "--qv", "out.qv", "--vcf", "out.vcf"]])
def test_guard_records_needs_the_entry_point(hypo_bin, tmp_path, extra):
    eu.build_shim()
    man = eu.make_inputs("e2e_20k_s1", tmp_path)
    argv = shlex.split(man["command"])
    argv[0] = hypo_bin
    argv += ["-o", "out.fa"]
    env = dict(os.environ, LD_LIBRARY_PATH=eu.SHIM_DIR + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
    p = subprocess.run(argv + ["--guard-records"] + extra, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode != 0
    assert "hypo_gpu_kset_query_variants" in p.stderr and "--guard-records" in p.stderr
    assert "BATCH-ID" not in p.stdout and "Solid kmers" not in p.stdout            # before any stage
    left = sorted(os.listdir(str(tmp_path)))
    assert not [f for f in left if f.startswith("out.") or f.endswith(".tmp")], left
