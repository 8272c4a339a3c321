"""`hypo --kmer-bridge` on the command line, without a GPU: the usage names the three flags behind --kmer-fix, the flag needs an
argument, --kmer-bridge-max and --kmer-bridge-slack refuse a value out of range and need --kmer-bridge, --qv-min-count takes the flag
as one of those it needs, and a device library without hypo_gpu_kset_query_walks (the CPU stand-in of tests/shim) ends the run before
any stage with an error that names the entry point and the flag, leaving no output and no .tmp behind, alone, next to --kmer-fix and
next to --qv, --vcf, --kmer-guard and --qv-bed."""
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


def hypo(hypo_bin, tmp_path, argv):
    return subprocess.run([hypo_bin] + argv, cwd=str(tmp_path), capture_output=True, text=True, timeout=60)


def nothing_left(tmp_path):
    return not [f for f in os.listdir(str(tmp_path)) if f != "aux"]


def test_usage_names_the_flags(hypo_bin, tmp_path):
    p = hypo(hypo_bin, tmp_path, ["-h"])
    assert p.returncode == 0
    fix = p.stdout.index("--kmer-fix <str>\n")
    i = p.stdout.index("--kmer-bridge <str>\n")
    j = p.stdout.index("--kmer-bridge-max <int>\n")
    l = p.stdout.index("--kmer-bridge-slack <int>\n")
    assert fix < i < j < l < p.stdout.index("-h, --help")
    what = p.stdout[i:j]
    assert "[MI355X build]" in what[:60] and "[Default] no bridges." in what
    for word in ("de Bruijn", "anchor", "exactly one walk", "--kmer-bridge-max", "--kmer-bridge-slack", "--kmer-fix", "--kmer-guard", "--qv-k", "--qv-min-count", "--vcf",
                 "pos", "missing k-mers", "steps"):
        assert word in what, word
    assert "[MI355X build]" in p.stdout[j:j + 60] and "2 to 192" in p.stdout[j:l] and "[Default] 64." in p.stdout[j:l]
    assert "[MI355X build]" in p.stdout[l:l + 60] and "0 to 64" in p.stdout[l:l + 400] and "[Default] 8." in p.stdout[l:l + 400]
    # the entry of --kmer-fix ends where it ended
    assert "[Default] no fixes.\n\n\t    --kmer-bridge <str>\n" in p.stdout


def test_flag_needs_an_argument(hypo_bin, tmp_path):
    for flag in ("kmer-bridge", "kmer-bridge-max", "kmer-bridge-slack"):
        p = hypo(hypo_bin, tmp_path, ["-c", "30", "--" + flag])
        assert "requires an argument" in p.stderr and flag in p.stderr
        assert "Usage: hypo <args>" in p.stdout
    assert nothing_left(tmp_path)


@pytest.mark.parametrize("flag,limits,bad", [("--kmer-bridge-max", ("2", "192"), ["1", "193", "x", "", "64x", "-3"]),
                                             ("--kmer-bridge-slack", ("0", "64"), ["65", "x", "-1", "8 "])])
def test_values_out_of_range(hypo_bin, tmp_path, flag, limits, bad):
    for v in bad:
        p = hypo(hypo_bin, tmp_path, ["--kmer-bridge", "b.tsv", flag, v])
        assert p.returncode == 1 and "Arg Error" in p.stderr and flag in p.stderr and all(x in p.stderr for x in limits), (v, p.stderr)
    for v in limits:
        p = hypo(hypo_bin, tmp_path, ["--kmer-bridge", "b.tsv", flag, v])
        assert "Arg Error" not in p.stderr and "Too few arguments" in p.stderr, (v, p.stderr)
    assert nothing_left(tmp_path)


def test_options_need_the_flag(hypo_bin, tmp_path):
    for argv in (["--kmer-bridge-max", "32"], ["--kmer-bridge-slack", "4"], ["--kmer-fix", "f.tsv", "--kmer-bridge-slack", "4", "--kmer-bridge-max", "32"]):
        p = hypo(hypo_bin, tmp_path, argv)
        assert p.returncode == 1 and "Arg Error" in p.stderr and "--kmer-bridge" in p.stderr and "Too few arguments" not in p.stderr, p.stderr
    p = hypo(hypo_bin, tmp_path, ["--kmer-bridge-max", "32", "--kmer-bridge-slack", "4", "--kmer-bridge", "b.tsv"])
    assert "Arg Error" not in p.stderr and "Too few arguments" in p.stderr
    assert nothing_left(tmp_path)


def test_min_count_accepts_the_flag(hypo_bin, tmp_path):
    for argv in (["--qv-min-count", "2", "--kmer-bridge", "f.tsv"], ["--kmer-bridge", "f.tsv", "--qv-min-count", "valley"]):
        p = hypo(hypo_bin, tmp_path, argv)
        assert "--qv-min-count" not in p.stderr and "Too few arguments" in p.stderr
    p = hypo(hypo_bin, tmp_path, ["--qv-min-count", "2"])
    assert p.returncode == 1 and "Arg Error" in p.stderr and "--kmer-fix" in p.stderr and "--guard-records" in p.stderr
    assert nothing_left(tmp_path)


@pytest.mark.parametrize("extra", [[], ["--kmer-fix", "out.fix.tsv"], ["--qv", "out.qv", "--vcf", "out.vcf", "--kmer-guard", "--qv-bed", "out.bed"]])
def test_bridge_needs_the_entry_point(hypo_bin, tmp_path, extra):
    eu.build_shim()
    man = eu.make_inputs("e2e_20k_s1", tmp_path)
    argv = shlex.split(man["command"])
    argv[0] = hypo_bin
    argv += ["-o", "out.fa"]
    env = dict(os.environ, LD_LIBRARY_PATH=eu.SHIM_DIR + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
    p = subprocess.run(argv + ["--kmer-bridge", "out.bridge.tsv"] + extra, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode != 0
    assert "hypo_gpu_kset_query_walks" in p.stderr and "--kmer-bridge" in p.stderr
    assert "BATCH-ID" not in p.stdout and "Solid kmers" not in p.stdout            # before any stage
    left = sorted(os.listdir(str(tmp_path)))
    assert not [f for f in left if f.startswith("out.") or f.endswith(".tmp")], left
