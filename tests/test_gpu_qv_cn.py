"""GPU: `hypo --qv-cn` end to end.  The file is the checker's text (tests/cn_checker.py) computed from the run's own reads and
output FASTA; the FASTA and every other output are those of the run without the flag, stdout differs only by the copy-number Info
line; the file is the same next to --qv-spectra (whose polished plane it then reads), from stage 1 and with --qv-load of the set the
first run saved; --qv-cn-unit at half and at twice the peak moves the calls as the checker says; --qv-min-count changes `missing`
as the checker says; with --kmer-guard and --kmer-fix the file describes the text in the FASTA; no .tmp is left."""
import os
import shlex
import shutil
import subprocess

import pytest

import cn_checker as cn
import e2e_util as eu
import edit_checker as ec
import spectra_checker as spc

pytestmark = pytest.mark.gpu
INFO = "[Hypo::Hypo] Info: copy number "


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(eu.BIN):
        eu.build_binary()


def run(argv, cwd):
    p = subprocess.run(argv, cwd=str(cwd), env=dict(os.environ, HYPO_REQUIRE_DEVICE="1"), capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert not [f for f in os.listdir(str(cwd)) if f.endswith(".tmp")]
    return p


def stable_stdout(text):
    """without the lines that carry a time, and without the line of this flag"""
    return sorted(l for l in text.splitlines() if not l.startswith("RESOURCES") and not l.startswith(INFO) and not l.startswith("[Hypo::Hypo] Info: k-mer set saved to "))


def golden_argv(name, tmp_path):
    man = eu.make_inputs(name, tmp_path)
    argv = shlex.split(man["command"])
    argv[0] = eu.BIN
    argv[argv.index("-t") + 1] = "16"
    return argv + ["-o", "out.fa"]


READS = {}


def read_counts(cwd, argv, k):
    """{k-mer: how often the reads have it, up to 255} of the run's read file, once per input"""
    path = os.path.join(str(cwd), argv[argv.index("-r") + 1])
    key = (eu._md5(path), k)
    if key not in READS:
        keys, counts = spc.read_counts([path], k)
        READS[key] = (keys, dict(zip(keys.tolist(), counts.tolist())))
    return READS[key]


def expected(cwd, argv, k, bin=1024, unit=None, t=1):
    """the checker's file for the run's own reads and output FASTA"""
    outs = ec.read_fastx(os.path.join(str(cwd), "out.fa"))
    keys, reads = read_counts(cwd, argv, k)
    copies, _ = spc.copy_numbers([s for _, s in outs], k, keys)
    text = {code: m for code, m in zip(keys.tolist(), copies.tolist()) if m}
    return cn.report([n for n, _ in outs], [s for _, s in outs], k, bin, reads, text, unit, t)


def check_info(stdout, name, text):
    assert [l for l in stdout.splitlines() if l.startswith(INFO)] == [cn.info_line(name, text)]


@pytest.mark.parametrize("name,k", [("e2e_20k_s1", None), ("e2e_5ctg_long_s21", 16)])
def test_cn_goldens(name, k, tmp_path):
    argv = golden_argv(name, tmp_path)
    assert "-i" in argv
    kk = 21 if k is None else k
    kargs = [] if k is None else ["--qv-k", str(k)]
    # stage 0 without and with the flag, --qv and --qv-spectra beside it (the plane --qv-spectra marks is read: no second mark)
    shutil.rmtree(os.path.join(str(tmp_path), "aux"), ignore_errors=True)
    p0 = run(argv + ["--qv", "q.tsv", "--qv-spectra", "s.tsv"] + kargs, tmp_path)
    files = ("out.fa", "q.tsv", "s.tsv")
    want = {f: (tmp_path / f).read_bytes() for f in files}
    shutil.rmtree(os.path.join(str(tmp_path), "aux"), ignore_errors=True)
    p = run(argv + ["--qv", "q.tsv", "--qv-spectra", "s.tsv", "--qv-cn", "cn0.tsv", "--qv-save", "set.bin"] + kargs, tmp_path)
    assert "Beginning from stage: 0" in p.stdout
    assert {f: (tmp_path / f).read_bytes() for f in files} == want
    assert stable_stdout(p.stdout) == stable_stdout(p0.stdout)
    text = (tmp_path / "cn0.tsv").read_text()
    assert text == expected(tmp_path, argv, kk)
    check_info(p.stdout, "cn0.tsv", text)
    r = cn.parse_report(text)
    assert (r["k"], r["bin"], r["how"], r["min_count"]) == (kk, 1024, "peak", 1) and 5 <= r["unit"] <= 60
    assert len({row[0] for row in r["rows"]}) == (5 if "5ctg" in name else 1) and sum(row[5] for row in r["rows"]) > 10000
    # from stage 1 and without --qv-spectra (the text is marked for this flag alone): the same file
    p1 = run(argv + ["--qv-cn", "cn1.tsv"] + kargs, tmp_path)
    assert "Beginning from stage: 1" in p1.stdout
    assert (tmp_path / "out.fa").read_bytes() == want["out.fa"] and (tmp_path / "cn1.tsv").read_text() == text
    check_info(p1.stdout, "cn1.tsv", text)
    # the set from the file the first run saved: no read is parsed for it, the same file
    p2 = run(argv + ["--qv-load", "set.bin", "--qv-cn", "cn2.tsv"] + kargs, tmp_path)
    assert "no read parsed for it" in p2.stderr
    assert (tmp_path / "out.fa").read_bytes() == want["out.fa"] and (tmp_path / "cn2.tsv").read_text() == text


def test_unit_at_half_and_twice_the_peak(tmp_path):
    argv = golden_argv("e2e_20k_s1", tmp_path)
    _, reads = read_counts(tmp_path, argv, 21)
    peak = cn.peak(cn.histogram(reads))
    assert peak >= 4
    calls = {}
    for unit in (peak // 2, 2 * peak):
        p = run(argv + ["--qv-cn", "cn.tsv", "--qv-cn-bin", "500", "--qv-cn-unit", str(unit)], tmp_path)
        text = (tmp_path / "cn.tsv").read_text()
        assert text == expected(tmp_path, argv, 21, bin=500, unit=unit)
        check_info(p.stdout, "cn.tsv", text)
        r = cn.parse_report(text)
        assert (r["unit"], r["how"], r["bin"]) == (unit, "given", 500)
        calls[unit] = [row[9] for row in r["rows"]]
    # what the checker gives at the peak itself, for comparison: a unit half as large calls more bins collapsed, one twice as large
    # more bins duplicated
    at_peak = [row[9] for row in cn.parse_report(expected(tmp_path, argv, 21, bin=500, unit=peak))["rows"]]
    assert calls[peak // 2].count("collapsed") > at_peak.count("collapsed") and calls[peak // 2].count("duplicated") == 0
    assert calls[2 * peak].count("duplicated") > at_peak.count("duplicated") and calls[2 * peak].count("collapsed") == 0


def test_min_count(tmp_path):
    argv = golden_argv("e2e_20k_s1", tmp_path)
    p = run(argv + ["--qv-cn", "cn.tsv", "--qv-cn-bin", "100", "--qv-min-count", "2"], tmp_path)
    text = (tmp_path / "cn.tsv").read_text()
    assert text == expected(tmp_path, argv, 21, bin=100, t=2)
    check_info(p.stdout, "cn.tsv", text)
    plain = cn.parse_report(expected(tmp_path, argv, 21, bin=100, t=1))
    got = cn.parse_report(text)
    assert got["min_count"] == 2 and got["unit"] == plain["unit"]
    assert sum(row[4] for row in got["rows"]) >= sum(row[4] for row in plain["rows"])


def test_beside_guard_fix_and_every_other_output(tmp_path):
    """--kmer-guard --kmer-fix --qv --qv-bed --vcf: every other output is what it is without --qv-cn, and the file describes the
    guarded and fixed text the FASTA holds"""
    argv = golden_argv("e2e_20k_s1", tmp_path) + ["--kmer-guard", "--kmer-fix", "o.fix", "--qv", "o.qv", "--qv-bed", "o.bed", "--vcf", "o.vcf"]
    p0 = run(argv, tmp_path)
    files = ("out.fa", "o.fix", "o.qv", "o.bed", "o.vcf")
    want = {f: (tmp_path / f).read_bytes() for f in files}
    p = run(argv + ["--qv-cn", "o.cn"], tmp_path)
    assert {f: (tmp_path / f).read_bytes() for f in files} == want
    assert stable_stdout(p.stdout) == stable_stdout(p0.stdout)
    text = (tmp_path / "o.cn").read_text()
    assert text == expected(tmp_path, argv, 21)
    check_info(p.stdout, "o.cn", text)
