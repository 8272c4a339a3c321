"""GPU: `hypo --qv-spectra` end to end.  The file is the checker's text (tests/spectra_checker.py) computed from the run's own
reads, draft and output FASTA; the FASTA and every other output are those of the run without the flag, stdout differs only by the
spectra Info line; asm_only_windows is the `*` row of --qv; a run from stage 1 and a -p 1 run write the same file; with
--kmer-guard the polished half describes the guarded FASTA; --qv-k below the solid k gets every window once; a given threshold is
reported and used; no .tmp is left."""
import os
import re
import shlex
import shutil
import subprocess

import pytest

import e2e_util as eu
import edit_checker as ec
import qv_checker as qc
import spectra_checker as spc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(eu.BIN):
        eu.build_binary()


def run(argv, cwd, env_extra=None):
    env = dict(os.environ, HYPO_REQUIRE_DEVICE="1")
    env.update(env_extra or {})
    p = subprocess.run(argv, cwd=str(cwd), env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert not [f for f in os.listdir(str(cwd)) if f.endswith(".tmp")]
    return p


def opt(argv, flag, default=None):
    return argv[argv.index(flag) + 1] if flag in argv else default


def stable_stdout(text):
    return sorted(l for l in text.splitlines() if not l.startswith("RESOURCES") and not l.startswith("[Hypo::Hypo] Info: spectra "))


def drop_aux(cwd):
    shutil.rmtree(os.path.join(str(cwd), "aux"), ignore_errors=True)


def golden_argv(name, tmp_path):
    man = eu.make_inputs(name, tmp_path)
    argv = shlex.split(man["command"])
    argv[0] = eu.BIN
    argv[argv.index("-t") + 1] = "16"
    return argv + ["-o", "out.fa"]


def expected(cwd, argv, k, reliable_min=None):
    """the checker's file for the run's own reads, draft and output FASTA"""
    path = lambda f: os.path.join(str(cwd), f)
    drafts, outs = ec.read_fastx(path(opt(argv, "-d"))), ec.read_fastx(path("out.fa"))
    assert [n for n, _ in outs] == [n for n, _ in drafts]
    return spc.report_for([path(opt(argv, "-r"))], k, [s for _, s in drafts], [s for _, s in outs], reliable_min)


def check_info(stdout, name, text):
    assert [l for l in stdout.splitlines() if l.startswith("[Hypo::Hypo] Info: spectra ")] == [spc.info_line(name, text)]


@pytest.mark.parametrize("name,k", [("e2e_20k_s1", None), ("e2e_5ctg_long_s21", 16)])
def test_spectra_goldens(name, k, tmp_path):
    argv = golden_argv(name, tmp_path)
    if name == "e2e_5ctg_long_s21":
        assert opt(argv, "-p") == "2"
    assert "-i" in argv
    kk = 21 if k is None else k
    kargs = [] if k is None else ["--qv-k", str(k)]
    # stage 0 without and with the flag (and --qv beside it)
    drop_aux(tmp_path)
    p0 = run(argv + ["--qv", "q.tsv"] + kargs, tmp_path)
    base, table = (tmp_path / "out.fa").read_bytes(), (tmp_path / "q.tsv").read_bytes()
    drop_aux(tmp_path)
    p = run(argv + ["--qv", "q.tsv", "--qv-spectra", "s0.tsv"] + kargs, tmp_path)
    assert "Beginning from stage: 0" in p.stdout and "the parse pass of the solid k-mers" in p.stderr
    assert (tmp_path / "out.fa").read_bytes() == base and (tmp_path / "q.tsv").read_bytes() == table
    assert stable_stdout(p.stdout) == stable_stdout(p0.stdout)
    text = (tmp_path / "s0.tsv").read_text()
    assert text == expected(tmp_path, argv, kk)
    check_info(p.stdout, "s0.tsv", text)
    r = spc.parse_report(text)
    star = qc.parse_table(table.decode())[-1]
    assert star[0] == "*" and (r["texts"]["draft"][3], r["texts"]["polished"][3]) == (star[1], star[4])
    assert r["how"] == "valley" and r["texts"]["polished"][0] > 1000 and r["texts"]["polished"][2] not in ("NA", "0.000000")
    # from stage 1 over the set that run stored the reads are parsed for the k-mer set alone; -p 1: the same file
    p1 = run(argv + ["--qv-spectra", "s1.tsv"] + kargs, tmp_path)
    assert "Beginning from stage: 1" in p1.stdout and "reads parsed for the QV alone" in p1.stderr
    assert (tmp_path / "out.fa").read_bytes() == base and (tmp_path / "s1.tsv").read_text() == text
    a1 = list(argv)
    if "-p" in a1:
        a1[a1.index("-p") + 1] = "1"
    else:
        a1 += ["-p", "1"]
    run(a1 + ["--qv-spectra", "sp1.tsv"] + kargs, tmp_path)
    assert (tmp_path / "out.fa").read_bytes() == base and (tmp_path / "sp1.tsv").read_text() == text


def test_spectra_beside_every_other_output(tmp_path):
    """--kmer-guard --qv --qv-bed --vcf: every other output is what it is without --qv-spectra, and the polished half of the file
    describes the guarded FASTA"""
    argv = golden_argv("e2e_20k_s1", tmp_path) + ["--kmer-guard", "--qv", "o.qv", "--qv-bed", "o.bed", "--vcf", "o.vcf"]
    p0 = run(argv, tmp_path)
    files = ("out.fa", "o.qv", "o.bed", "o.vcf")
    want = {f: (tmp_path / f).read_bytes() for f in files}
    p = run(argv + ["--qv-spectra", "o.tsv"], tmp_path)
    assert {f: (tmp_path / f).read_bytes() for f in files} == want
    assert stable_stdout(p.stdout) == stable_stdout(p0.stdout)
    text = (tmp_path / "o.tsv").read_text()
    assert text == expected(tmp_path, argv, 21)
    star = qc.parse_table(want["o.qv"].decode())[-1]
    assert spc.parse_report(text)["texts"]["polished"][3] == star[4]


def test_qv_k_below_the_solid_k(tmp_path):
    """--qv-k 12 on a set whose solid k is 13 (-s 100m), the reads in chunks of 64 KiB: the chunks overlap by 12 bytes, the set gets
    each from its own 11 bytes before the new ones, and no window is counted twice"""
    eu._gen().generate(str(tmp_path), 7, 60000, False, 5)
    argv = [eu.BIN, "-d", "draft.fa", "-r", "reads.fa", "-s", "100m", "-c", "30", "-b", "sr.sam", "-t", "16", "-o", "out.fa"]
    p = run(argv + ["--qv-k", "12", "--qv-spectra", "s.tsv"], tmp_path, {"HYPO_READ_CHUNK_KB": "64"})
    assert "Value of K chosen for the given genome size (100m): 13" in p.stdout
    assert os.path.getsize(str(tmp_path / "reads.fa")) > 20 * 65536
    text = (tmp_path / "s.tsv").read_text()
    assert text == expected(tmp_path, argv, 12)
    # ... and one chunk gives the same file
    run(argv + ["--qv-k", "12", "--qv-spectra", "s1.tsv"], tmp_path)
    assert (tmp_path / "s1.tsv").read_text() == text


def test_given_threshold(tmp_path):
    argv = golden_argv("e2e_20k_s1", tmp_path)
    p = run(argv + ["--qv-spectra", "s.tsv", "--qv-reliable-min", "7"], tmp_path)
    text = (tmp_path / "s.tsv").read_text()
    assert text == expected(tmp_path, argv, 21, reliable_min=7)
    r = spc.parse_report(text)
    assert (r["reliable_min"], r["how"]) == (7, "given") and "reliable >= 7" in p.stdout
    assert r["texts"]["draft"][:3] == spc.completeness(r["draft"], 7)
    check_info(p.stdout, "s.tsv", text)
