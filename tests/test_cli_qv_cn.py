"""`hypo --qv-cn` on the command line, without a GPU: the usage names the three flags, each needs its argument, --qv-cn-bin and
--qv-cn-unit are range-checked and need --qv-cn, all before anything is created, and a device library without
hypo_gpu_kset_query_depth (the CPU stand-in of tests/shim) ends the run before any stage with an error that names the entry point
and the flag, leaving no output and no .tmp behind, alone and next to --qv-spectra."""
import os
import shlex
import subprocess

import pytest

import e2e_util as eu


@pytest.fixture(scope="module")
def hypo_bin():
    return eu.build_binary()                                               # (a build that fails fails these tests)


def hypo(hypo_bin, cwd, args, **kw):
    return subprocess.run([hypo_bin] + args, cwd=str(cwd), capture_output=True, text=True, timeout=kw.pop("timeout", 60), **kw)


def test_usage_names_the_flags(hypo_bin, tmp_path):
    p = hypo(hypo_bin, tmp_path, ["-h"])
    assert p.returncode == 0
    i, j, u, h = (p.stdout.index(s) for s in ("--qv-cn <str>\n", "--qv-cn-bin <int>\n", "--qv-cn-unit <int>\n", "-h, --help"))
    assert p.stdout.index("--kmer-bridge-vote <int>\n") < i < j < u < h             # behind the last flag there was
    what = p.stdout[i:j]
    assert "[MI355X build]" in what[:60] and "[Default] no copy-number file." in what
    for word in ("collapsed", "duplicated", "1.5 times", "0.75 times", "median", "one byte a base", "--qv-cn-bin", "--qv-cn-unit", "--qv-k", "--qv-mem",
                 "--qv-min-count", "--qv-save", "--qv-load"):
        assert word in what, word
    what = p.stdout[j:u]
    assert "[MI355X build]" in what[:60] and "32 to 65536" in what and "Needs --qv-cn." in what and "[Default] 1024." in what
    what = p.stdout[u:h]
    assert "[MI355X build]" in what[:60] and "1 to 255" in what and "Needs --qv-cn." in what and "[Default] the peak of the read k-mer histogram" in what
    # the entry of --kmer-bridge-vote ends where it ended
    assert "[Default] no vote.\n\n\t    --qv-cn <str>\n" in p.stdout


@pytest.mark.parametrize("flag", ["--qv-cn", "--qv-cn-bin", "--qv-cn-unit"])
def test_flags_need_an_argument(hypo_bin, tmp_path, flag):
    p = hypo(hypo_bin, tmp_path, ["-c", "30", flag])
    assert "requires an argument" in p.stderr and flag[2:] in p.stderr
    assert "Usage: hypo <args>" in p.stdout
    assert not [f for f in os.listdir(str(tmp_path)) if f != "aux"]


@pytest.mark.parametrize("flag,v", [("--qv-cn-bin", v) for v in ("31", "65537", "0", "-5", "x", "1k", "")] +
                                   [("--qv-cn-unit", v) for v in ("0", "256", "-1", "x", "7x", "")])
def test_out_of_range(hypo_bin, tmp_path, flag, v):
    p = hypo(hypo_bin, tmp_path, ["--qv-cn", "out.tsv", flag, v])
    lo, hi = ("32", "65536") if flag == "--qv-cn-bin" else ("1", "255")
    assert p.returncode == 1
    assert flag in p.stderr and lo in p.stderr and hi in p.stderr
    assert not os.listdir(str(tmp_path))


@pytest.mark.parametrize("args", [["--qv-cn-bin", "32"], ["--qv-cn-bin", "65536"], ["--qv-cn-unit", "1"], ["--qv-cn-unit", "255"]])
def test_in_range_is_accepted(hypo_bin, tmp_path, args):
    p = hypo(hypo_bin, tmp_path, ["--qv-cn", "out.tsv"] + args)
    assert "--qv-cn" not in p.stderr and "Too few arguments" in p.stderr


@pytest.mark.parametrize("args", [["--qv-cn-bin", "100"], ["--qv-cn-unit", "30"], ["--qv-cn-bin", "100", "--qv-cn-unit", "30", "--qv-spectra", "s.tsv"]])
def test_the_two_need_qv_cn(hypo_bin, tmp_path, args):
    p = hypo(hypo_bin, tmp_path, args)
    assert p.returncode == 1
    assert "--qv-cn-bin" in p.stderr and "--qv-cn-unit" in p.stderr and "need --qv-cn" in p.stderr
    assert not os.listdir(str(tmp_path))


def test_qv_cn_is_a_flag_that_asks_the_set(hypo_bin, tmp_path):
    """--qv-min-count and --qv-load need a flag that asks the set: --qv-cn alone is one"""
    for extra in (["--qv-min-count", "3"], ["--qv-load", "set.bin"]):
        p = hypo(hypo_bin, tmp_path, ["--qv-cn", "out.tsv"] + extra)
        assert "Too few arguments" in p.stderr and "needs at least one" not in p.stderr, p.stderr
        q = hypo(hypo_bin, tmp_path, extra)
        assert q.returncode == 1 and "needs at least one" in q.stderr


@pytest.mark.parametrize("extra", [[], ["--qv-cn-bin", "100", "--qv-cn-unit", "30"], ["--qv-spectra", "out.spectra"],
                                   ["--qv", "out.qv", "--qv-bed", "out.bed", "--qv-spectra", "out.spectra", "--kmer-guard"]])
def test_cn_needs_the_entry_point(hypo_bin, tmp_path, extra):
    eu.build_shim()
    man = eu.make_inputs("e2e_20k_s1", tmp_path)
    argv = shlex.split(man["command"])[1:] + ["-o", "out.fa"]
    env = dict(os.environ, LD_LIBRARY_PATH=eu.SHIM_DIR + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
    p = hypo(hypo_bin, tmp_path, argv + ["--qv-cn", "out.cn"] + extra, env=env, timeout=300)
    assert p.returncode != 0
    assert "hypo_gpu_kset_query_depth" in p.stderr and "--qv-cn" in p.stderr, p.stderr
    assert "BATCH-ID" not in p.stdout and "Solid kmers" not in p.stdout            # before any stage
    left = sorted(os.listdir(str(tmp_path)))
    assert not [f for f in left if f.startswith("out.") or f.endswith(".tmp")], left
