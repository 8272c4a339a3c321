"""`hypo --kmer-bridge-vote` on the command line, without a GPU: the usage names the flag behind --kmer-bridge-slack, the flag needs an
argument, refuses a ratio out of 2..255 and needs --kmer-bridge, and a device library without hypo_gpu_kset_query_walk_sets (the CPU
stand-in of tests/shim) ends the run before any stage with an error that names the entry point and the flag, leaving no output and no
.tmp behind, alone and next to --kmer-fix, --qv and --vcf."""
import os
import shlex
import subprocess

import pytest

import e2e_util as eu
from test_cli_kmer_bridge import hypo, nothing_left


@pytest.fixture(scope="module")
def hypo_bin():
    return eu.build_binary()                                               # (a build that fails fails these tests)


def test_usage_names_the_flag(hypo_bin, tmp_path):
    p = hypo(hypo_bin, tmp_path, ["-h"])
    assert p.returncode == 0
    l = p.stdout.index("--kmer-bridge-slack <int>\n")
    v = p.stdout.index("--kmer-bridge-vote <int>\n")
    h = p.stdout.index("-h, --help")
    assert l < v < h
    what = p.stdout[v:h]
    assert "[MI355X build]" in what[:60] and "[Default] no vote." in what
    for word in ("ambiguous", "up to 4 walks", "support", "2 to 255", "at least this many times", "heterozygous", "more than 4 walks", "walks found", "best/second",
                 "--qv-min-count", "--qv-mem", "Needs --kmer-bridge."):
        assert word in what, word
    # the entry of --kmer-bridge-slack ends where it ended
    assert "[Default] 8.\n\n\t    --kmer-bridge-vote <int>\n" in p.stdout


def test_flag_needs_an_argument(hypo_bin, tmp_path):
    p = hypo(hypo_bin, tmp_path, ["-c", "30", "--kmer-bridge-vote"])
    assert "requires an argument" in p.stderr and "kmer-bridge-vote" in p.stderr
    assert "Usage: hypo <args>" in p.stdout
    assert nothing_left(tmp_path)


def test_values_out_of_range(hypo_bin, tmp_path):
    for v in ("1", "256", "x", "", "4x", "0", "-4"):
        p = hypo(hypo_bin, tmp_path, ["--kmer-bridge", "b.tsv", "--kmer-bridge-vote", v])
        assert p.returncode == 1 and "Arg Error" in p.stderr and "--kmer-bridge-vote" in p.stderr and "2" in p.stderr and "255" in p.stderr, (v, p.stderr)
        assert "Too few arguments" not in p.stderr
    for v in ("2", "255"):
        p = hypo(hypo_bin, tmp_path, ["--kmer-bridge", "b.tsv", "--kmer-bridge-vote", v])
        assert "Arg Error" not in p.stderr and "Too few arguments" in p.stderr, (v, p.stderr)
    assert nothing_left(tmp_path)


def test_needs_kmer_bridge(hypo_bin, tmp_path):
    for argv in (["--kmer-bridge-vote", "4"], ["--kmer-fix", "f.tsv", "--qv-min-count", "2", "--kmer-bridge-vote", "4"]):
        p = hypo(hypo_bin, tmp_path, argv)
        assert p.returncode == 1 and "Arg Error" in p.stderr and "Too few arguments" not in p.stderr, p.stderr
        assert "--kmer-bridge-vote" in p.stderr and "needs --kmer-bridge!" in p.stderr and "2 to 255" in p.stderr
    for argv in (["--kmer-bridge-vote", "4", "--kmer-bridge", "b.tsv"], ["--kmer-bridge", "b.tsv", "--qv-min-count", "2", "--kmer-bridge-vote", "4"]):
        p = hypo(hypo_bin, tmp_path, argv)
        assert "Arg Error" not in p.stderr and "Too few arguments" in p.stderr
    assert nothing_left(tmp_path)


@pytest.mark.parametrize("extra", [[], ["--kmer-fix", "out.fix.tsv", "--qv", "out.qv", "--vcf", "out.vcf"]])
def test_vote_needs_the_entry_point(hypo_bin, tmp_path, extra):
    eu.build_shim()
    man = eu.make_inputs("e2e_20k_s1", tmp_path)
    argv = shlex.split(man["command"])
    argv[0] = hypo_bin
    argv += ["-o", "out.fa"]
    env = dict(os.environ, LD_LIBRARY_PATH=eu.SHIM_DIR + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
    p = subprocess.run(argv + ["--kmer-bridge", "out.bridge.tsv", "--kmer-bridge-vote", "4"] + extra, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode != 0
    assert "hypo_gpu_kset_query_walk_sets" in p.stderr and "--kmer-bridge-vote" in p.stderr
    assert "BATCH-ID" not in p.stdout and "Solid kmers" not in p.stdout            # before any stage
    left = sorted(os.listdir(str(tmp_path)))
    assert not [f for f in left if f.startswith("out.") or f.endswith(".tmp")], left
