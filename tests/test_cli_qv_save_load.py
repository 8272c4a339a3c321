"""`hypo --qv-save / --qv-load` on the command line, without a GPU: the usage names the two flags behind --qv-mem, each needs an
argument, the two together and --qv-load without a flag that asks the set are Arg Errors, and a device library without
hypo_gpu_kset_export / hypo_gpu_kset_import (the CPU stand-in of tests/shim) ends the run before any stage with an error that names
the entry point and the flag, leaving no output, no set file and no .tmp behind."""
import os
import shlex
import subprocess

import pytest

import e2e_util as eu


@pytest.fixture(scope="module")
def hypo_bin():
    return eu.build_binary()                                             # (a build that fails fails these tests)


def hypo(hypo_bin, tmp_path, argv):
    return subprocess.run([hypo_bin] + argv, cwd=str(tmp_path), capture_output=True, text=True, timeout=60)


def nothing_left(tmp_path):
    return not [f for f in os.listdir(str(tmp_path)) if f != "aux"]


def test_usage_names_the_flags(hypo_bin, tmp_path):
    p = hypo(hypo_bin, tmp_path, ["-h"])
    assert p.returncode == 0
    mem = p.stdout.index("--qv-mem <GiB>\n")
    i = p.stdout.index("--qv-save <str>\n")
    j = p.stdout.index("--qv-load <str>\n")
    guard = p.stdout.index("--kmer-guard\n")
    assert mem < i < j < guard < p.stdout.index("-h, --help")
    save, load = p.stdout[i:j], p.stdout[j:guard]
    assert "[MI355X build]" in save[:60] and "[Default] the set is not stored." in save
    for word in ("k-mer set", "before any contig is polished", "--qv-min-count", "--qv-mem", ".tmp", "255"):
        assert word in save, word
    assert "[MI355X build]" in load[:60] and "[Default] the set is built from the reads." in load
    for word in ("--qv-save", "not parsed", "byte for byte", "--qv-k", "digest", "--qv", "--kmer-guard", "--kmer-bridge"):
        assert word in load, word
    # the entry of --qv-mem ends where it ended
    assert "[Default] half of the device's free memory.\n\n\t    --qv-save <str>\n" in p.stdout


def test_flags_need_an_argument(hypo_bin, tmp_path):
    for flag in ("qv-save", "qv-load"):
        p = hypo(hypo_bin, tmp_path, ["-c", "30", "--" + flag])
        assert "requires an argument" in p.stderr and flag in p.stderr
        assert "Usage: hypo <args>" in p.stdout
    assert nothing_left(tmp_path)


def test_both_flags_are_an_arg_error(hypo_bin, tmp_path):
    for argv in (["--qv-save", "a.hks", "--qv-load", "b.hks", "--qv", "q.tsv"], ["--qv-load", "b.hks", "--kmer-guard", "--qv-save", "a.hks"]):
        p = hypo(hypo_bin, tmp_path, argv)
        assert p.returncode == 1 and "Arg Error" in p.stderr and "--qv-save" in p.stderr and "--qv-load" in p.stderr and "Too few arguments" not in p.stderr, p.stderr
    assert nothing_left(tmp_path)


def test_load_needs_a_flag_that_asks_the_set(hypo_bin, tmp_path):
    for argv in (["--qv-load", "b.hks"], ["--qv-load", "b.hks", "--vcf", "v.vcf", "--qv-k", "31"]):
        p = hypo(hypo_bin, tmp_path, argv)
        assert p.returncode == 1 and "Arg Error" in p.stderr and "--qv-load" in p.stderr and "Too few arguments" not in p.stderr, p.stderr
        for flag in ("--qv,", "--qv-bed", "--qv-spectra", "--kmer-guard", "--kmer-fix", "--kmer-bridge"):
            assert flag in p.stderr, flag
    # every flag that asks the set serves, and --qv-save needs none
    for argv in (["--qv-load", "b.hks", "--qv", "q.tsv"], ["--qv-load", "b.hks", "--qv-bed", "q.bed"], ["--qv-load", "b.hks", "--qv-spectra", "q.sp"],
                 ["--qv-load", "b.hks", "--kmer-guard"], ["--qv-load", "b.hks", "--guard-records"], ["--kmer-fix", "f.tsv", "--qv-load", "b.hks"],
                 ["--kmer-bridge", "b.tsv", "--qv-load", "b.hks"], ["--qv-save", "a.hks"]):
        p = hypo(hypo_bin, tmp_path, argv)
        assert "Arg Error" not in p.stderr and "Too few arguments" in p.stderr, (argv, p.stderr)
    assert nothing_left(tmp_path)


def shim_run(hypo_bin, tmp_path, extra):
    eu.build_shim()
    man = eu.make_inputs("e2e_20k_s1", tmp_path)
    argv = shlex.split(man["command"])
    argv[0] = hypo_bin
    argv += ["-o", "out.fa"]
    env = dict(os.environ, LD_LIBRARY_PATH=eu.SHIM_DIR + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
    return subprocess.run(argv + extra, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)


def left_behind(tmp_path):
    left = sorted(os.listdir(str(tmp_path)))
    return [f for f in left if f.startswith("out.") or f.endswith(".tmp") or f.endswith(".hks")]


@pytest.mark.parametrize("extra", [[], ["--qv", "out.qv"], ["--qv", "out.qv", "--vcf", "out.vcf", "--kmer-guard", "--kmer-bridge", "out.bridge.tsv"]])
def test_save_needs_the_entry_point(hypo_bin, tmp_path, extra):
    p = shim_run(hypo_bin, tmp_path, ["--qv-save", "set.hks"] + extra)
    assert p.returncode != 0
    assert "hypo_gpu_kset_export" in p.stderr and "--qv-save" in p.stderr and "does not provide" in p.stderr
    assert "BATCH-ID" not in p.stdout and "Solid kmers" not in p.stdout            # before any stage
    assert not left_behind(tmp_path)


@pytest.mark.parametrize("extra", [["--qv", "out.qv"], ["--kmer-guard", "--qv-bed", "out.bed", "--kmer-fix", "out.fix.tsv"]])
def test_load_needs_the_entry_point(hypo_bin, tmp_path, extra):
    # (the file does not exist: the entry point is looked for first)
    p = shim_run(hypo_bin, tmp_path, ["--qv-load", "set.hks"] + extra)
    assert p.returncode != 0
    assert "hypo_gpu_kset_import" in p.stderr and "--qv-load" in p.stderr and "does not provide" in p.stderr
    assert "BATCH-ID" not in p.stdout and "Solid kmers" not in p.stdout
    assert not left_behind(tmp_path)
