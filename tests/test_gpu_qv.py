"""GPU: `hypo --qv` end to end.  For every set: the FASTA is the one the run without --qv writes (and the golden's), stdout differs
only by the QV Info line and timings, no .tmp is left, the integer columns of the table are the checker's (tests/qv_checker.py)
computed from the run's own reads, draft and output FASTA, the printed QVs are the formula applied to those integers, -p 1 writes
the same table, and so does a -i run that starts from stage 1 and parses the reads for the QV alone."""
import gzip
import hashlib
import math
import os
import re
import shlex
import shutil
import subprocess

import pytest

import e2e_util as eu
import edit_checker as ec
import qv_checker as qc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(eu.BIN):
        eu.build_binary()


def run(argv, cwd, env_extra=None):
    env = dict(os.environ, HYPO_REQUIRE_DEVICE="1")
    env.update(env_extra or {})
    p = subprocess.run(argv, cwd=str(cwd), env=env, capture_output=True, text=True, timeout=1800)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return p


def opt(argv, flag, default=None):
    return argv[argv.index(flag) + 1] if flag in argv else default


def stable_stdout(text):
    return [l for l in text.splitlines() if not l.startswith("RESOURCES") and not l.startswith("[Hypo::Hypo] Info: QV ")]


def drop_aux(cwd):
    shutil.rmtree(os.path.join(str(cwd), "aux"), ignore_errors=True)


def check_table(text, k, reads, draft_path, fasta_path, info):
    """the table against the checker; info = (k, distinct, draft qv, polished qv) of the stdout line"""
    R = qc.read_set(reads, k)
    drafts, outs = ec.read_fastx(draft_path), ec.read_fastx(fasta_path)
    assert [n for n, _ in outs] == [n for n, _ in drafts]
    want = qc.rows(drafts, outs, k, R)
    got = qc.parse_table(text)
    assert [(r[0], r[1], r[2], r[4], r[5]) for r in got] == want
    for name, dm, dt, dqv, pm, pt, pqv in got:
        for printed, m, t in ((dqv, dm, dt), (pqv, pm, pt)):
            v = qc.qv_value(m, t, k)
            if v is None or v == math.inf:
                assert printed == ("NA" if v is None else "inf")
            else:
                assert re.fullmatch(r"\d+\.\d\d", printed) and abs(float(printed) - v) <= 0.005 + 1e-9, (name, printed, v)
    assert text == qc.table(want, k)
    assert int(info[0]) == k and int(info[1]) == R.size
    assert (info[2], info[3]) == (got[-1][3], got[-1][6])
    return want


def check_qv_run(argv, cwd, k=None, fasta_md5=None):
    """argv: a command line with -i (argv[0] = the binary).  With fasta_md5 the set came with its own aux/ (the generator derives
    that solid set from the truth, not from the reads, so the golden FASTA belongs to the run that loads it): first that run, from
    stage 1, without and with --qv.  Then aux/ is dropped: stage 0 without and with --qv, from stage 1 over the set stage 0
    stored, and -p 1."""
    assert "-i" in argv
    base_name = os.path.basename(opt(argv, "-d"))
    out = opt(argv, "-o", "hypo_" + (base_name[:base_name.rfind(".")] if "." in base_name else base_name) + ".fasta")
    out_path = os.path.join(str(cwd), out)
    kk = 21 if k is None else k
    qv_args = lambda f: ["--qv", f] + ([] if k is None else ["--qv-k", str(k)])
    path = lambda f: os.path.join(str(cwd), f)
    reads = opt(argv, "-r")
    read_paths = [reads if reads.startswith("@") else path(reads)]

    def pair(tag, stage, note):
        """the run without and with the flag, both from `stage`; the table checked against the checker"""
        if stage == 0:
            drop_aux(cwd)
        p0 = run(argv, cwd)
        assert f"Beginning from stage: {stage}" in p0.stdout
        base = open(out_path, "rb").read()
        os.replace(out_path, out_path + ".noqv")
        if stage == 0:
            drop_aux(cwd)
        p = run(argv + qv_args(tag + ".tsv"), cwd)
        assert f"Beginning from stage: {stage}" in p.stdout
        assert open(out_path, "rb").read() == base, "--qv changed the FASTA"
        # (as multisets: the long-read loader prints from its own thread, so its lines may land between others in either run)
        assert sorted(stable_stdout(p.stdout)) == sorted(stable_stdout(p0.stdout))
        info = re.findall(r"\[Hypo::Hypo\] Info: QV " + tag + r"\.tsv \(k = (\d+), (\d+) distinct read k-mers\): draft (\S+), polished (\S+)$", p.stdout, flags=re.M)
        assert len(info) == 1, p.stdout[-1500:]
        assert note in p.stderr
        assert not [f for f in os.listdir(str(cwd)) if f.endswith(".tmp")]
        table = open(path(tag + ".tsv")).read()
        want = check_table(table, kk, read_paths, path(opt(argv, "-d")), out_path, info[0])
        return base, table, want

    if fasta_md5:
        assert os.path.exists(path("aux/stage.txt"))
        base, _, _ = pair("qg", 1, "reads parsed for the QV alone")
        assert hashlib.md5(base).hexdigest() == fasta_md5, "polished FASTA differs from the golden"
    # stage 0: the reads are parsed once, for the solid k-mers and the set
    base, table, want = pair("q0", 0, "the parse pass of the solid k-mers")
    # from stage 1 over the set that run stored: the reads are parsed for the QV alone, the table is the same
    p1 = run(argv + qv_args("q1.tsv"), cwd)
    assert "Beginning from stage: 1" in p1.stdout and "reads parsed for the QV alone" in p1.stderr
    assert open(out_path, "rb").read() == base
    assert open(path("q1.tsv")).read() == table
    # -p 1
    a1 = list(argv)
    if "-p" in a1:
        a1[a1.index("-p") + 1] = "1"
    else:
        a1 += ["-p", "1"]
    run(a1 + qv_args("qp1.tsv"), cwd)
    assert open(path("qp1.tsv")).read() == table
    assert not [f for f in os.listdir(str(cwd)) if f.endswith(".tmp")]
    return table, want


def golden_argv(name, tmp_path):
    man = eu.make_inputs(name, tmp_path)
    argv = shlex.split(man["command"])
    argv[0] = eu.BIN
    argv[argv.index("-t") + 1] = "16"
    return man, argv


@pytest.mark.parametrize("name,k", [("e2e_20k_s1", None), ("e2e_200k_long_s3", None), ("e2e_5ctg_long_s21", 16)])
def test_qv_goldens(name, k, tmp_path):
    """a plain set, a -B set and a multi-contig -p 2 set"""
    man, argv = golden_argv(name, tmp_path)
    if name == "e2e_5ctg_long_s21":
        assert opt(argv, "-p") == "2"
    if name == "e2e_200k_long_s3":
        assert "-B" in argv
    table, want = check_qv_run(argv, tmp_path, k=k, fasta_md5=man["expected_fasta_md5"])
    assert want[-1][2] > 0 and want[-1][4] > 0


def test_qv_k13_set(tmp_path):
    """a set whose solid k is 13 (-s 100m), as tests/test_gpu_solid_build.py generates it"""
    eu._gen().generate(str(tmp_path), 7, 60000, False, 5)
    argv = [eu.BIN, "-d", "draft.fa", "-r", "reads.fa", "-s", "100m", "-c", "30", "-b", "sr.sam", "-t", "16", "-i"]
    check_qv_run(argv, tmp_path)
    assert "Value of K chosen for the given genome size (100m): 13" in run(argv, tmp_path).stdout


def test_qv_read_formats_and_k_values(tmp_path):
    """the reads as gzipped multi-line FASTQ plus FASTA behind an @list give the table of the plain file, at k = 12, 22 and 31"""
    man, argv = golden_argv("e2e_20k_s1", tmp_path)
    argv.remove("-i")
    recs = ec.read_fastx(str(tmp_path / "reads.fa"))
    h = len(recs) // 2
    (tmp_path / "a.fq.gz").write_bytes(gzip.compress("".join(
        f"@{n} x\n{s[:70]}\n{s[70:]}\n+\n{'I' * len(s[:70])}\n{'I' * len(s[70:])}\n" for n, s in recs[:h]).encode()))
    (tmp_path / "b.fa").write_text("".join(f">{n}\n" + "\n".join(s[j:j + 60] for j in range(0, len(s), 60)) + "\n" for n, s in recs[h:]))
    (tmp_path / "list.txt").write_text("a.fq.gz\nb.fa\n")
    listed = list(argv)
    listed[listed.index("-r") + 1] = "@list.txt"
    for k in (12, 22, 31):
        drop_aux(tmp_path)
        p = run(argv + ["--qv", f"plain{k}.tsv", "--qv-k", str(k)], tmp_path)
        info = re.findall(r"Info: QV \S+ \(k = (\d+), (\d+) distinct read k-mers\): draft (\S+), polished (\S+)$", p.stdout, flags=re.M)
        plain = (tmp_path / f"plain{k}.tsv").read_text()
        check_table(plain, k, [str(tmp_path / "reads.fa")], str(tmp_path / "draft.fa"), str(tmp_path / "hypo_draft.fasta"), info[0])
        drop_aux(tmp_path)
        run(listed + ["--qv", f"list{k}.tsv", "--qv-k", str(k)], tmp_path)
        assert (tmp_path / f"list{k}.tsv").read_text() == plain


def test_qv_with_vcf(tmp_path):
    man, argv = golden_argv("e2e_200k_long_s3", tmp_path)
    run(argv + ["--qv", "alone.tsv"], tmp_path)
    run(argv + ["--vcf", "alone.vcf"], tmp_path)
    p = run(argv + ["--qv", "both.tsv", "--vcf", "both.vcf"], tmp_path)
    assert (tmp_path / "both.tsv").read_bytes() == (tmp_path / "alone.tsv").read_bytes()
    assert (tmp_path / "both.vcf").read_bytes() == (tmp_path / "alone.vcf").read_bytes()
    assert eu.fasta_md5(tmp_path) == man["expected_fasta_md5"]
    assert "Info: VCF both.vcf" in p.stdout and "Info: QV both.tsv" in p.stdout
    assert not [f for f in os.listdir(str(tmp_path)) if f.endswith(".tmp")]


def test_qv_cap_ends_the_run_before_polishing(tmp_path):
    """--qv-mem below what the reads need: an error that names the size reached, before any contig is polished, no output"""
    man, argv = golden_argv("e2e_20k_s1", tmp_path)
    env = dict(os.environ, HYPO_REQUIRE_DEVICE="1")
    for with_aux in (True, False):
        if not with_aux:
            drop_aux(tmp_path)
        p = subprocess.run(argv + ["-o", "out.fa", "--qv", "out.tsv", "--vcf", "out.vcf", "--qv-mem", "0.0001"], cwd=str(tmp_path), env=env,
                           capture_output=True, text=True, timeout=600)
        assert p.returncode == 1
        assert "[Hypo::QV] Error" in p.stderr and "GiB" in p.stderr and "--qv-mem" in p.stderr and "distinct" in p.stderr
        assert "BATCH-ID" not in p.stdout
        assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("out.")]
