"""GPU: `hypo --vcf` end to end.  For every set: the FASTA is the one the run without --vcf writes (and the golden's), stdout differs
only by the VCF Info line and timings, the VCF applied to the draft gives the FASTA, and the VCF is byte for byte the one the
checker (tests/edit_checker.py) derives from the draft and the run's HYPO_REGION_DUMP file; -p 1 writes the same VCF."""
import hashlib
import importlib.util
import os
import re
import shlex
import subprocess

import pytest

import e2e_util as eu
import edit_checker as ec

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(eu.BIN):
        eu.build_binary()


def norm_draft(seq):
    return "".join(c if c in "ACGT" else "N" for c in seq.upper())


def run(argv, cwd, env_extra=None):
    env = dict(os.environ, HYPO_REQUIRE_DEVICE="1", HYPO_REGION_DUMP=os.path.join(str(cwd), "regions.tsv"))
    env.update(env_extra or {})
    p = subprocess.run(argv, cwd=str(cwd), env=env, capture_output=True, text=True, timeout=1800)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return p


def opt(argv, flag, default=None):
    return argv[argv.index(flag) + 1] if flag in argv else default


def stable_stdout(text):
    return [l for l in text.splitlines() if not l.startswith("RESOURCES") and not l.startswith("[Hypo::Hypo] Info: VCF ")]


def check_vcf_run(argv, cwd, env_extra=None, fasta_md5=None, p1=True):
    """argv: the run's command line (argv[0] = the binary).  Runs it without and with --vcf and checks everything.  Every compared
    run starts from the same stage: with -i, a first run stores stage 1 when the set did not come with it."""
    base_name = os.path.basename(opt(argv, "-d"))
    out = opt(argv, "-o", "hypo_" + (base_name[:base_name.rfind(".")] if "." in base_name else base_name) + ".fasta")
    out_path = os.path.join(str(cwd), out)

    def run_(a):
        return run(a, cwd, env_extra)
    if "-i" in argv and not os.path.exists(os.path.join(str(cwd), "aux", "stage.txt")):
        run_(argv)
    p0 = run_(argv)
    base = open(out_path, "rb").read()
    if fasta_md5:
        assert hashlib.md5(base).hexdigest() == fasta_md5, "polished FASTA differs from the golden"
    os.rename(out_path, out_path + ".novcf")
    p = run_(argv + ["--vcf", "edits.vcf"])
    got = open(out_path, "rb").read()
    assert got == base, "--vcf changed the FASTA"
    # (as multisets: the long-read loader prints from its own thread, so its lines may land between others in either run)
    assert sorted(stable_stdout(p.stdout)) == sorted(stable_stdout(p0.stdout))
    info = re.findall(r"\[Hypo::Hypo\] Info: VCF edits\.vcf: (\d+) records, (\d+) substituted, (\d+) inserted, (\d+) deleted bases", p.stdout)
    assert len(info) == 1, p.stdout[-1500:]
    vcf = open(os.path.join(str(cwd), "edits.vcf")).read()
    assert not os.path.exists(os.path.join(str(cwd), "edits.vcf.tmp"))
    # (2) the VCF applied to the draft is the FASTA
    drafts = [(n, norm_draft(s)) for n, s in ec.read_fastx(os.path.join(str(cwd), opt(argv, "-d")))]
    outs = ec.read_fastx(out_path)
    assert [n for n, _ in outs] == [n for n, _ in drafts]
    head, recs = ec.parse_vcf(vcf)
    assert f"##reference={opt(argv, '-d')}" in head
    n_rec = 0
    for (name, d), (_, o) in zip(drafts, outs):
        r = recs.get(name, [])
        n_rec += len(r)
        assert ec.apply(r, d) == o, f"{name}: VCF applied to the draft differs from the FASTA"
    assert n_rec == int(info[0][0])
    # (3) the checker's VCF from the draft and the region dump
    dmap = dict(drafts)
    units, rebuilt = ec.units_from_dump(os.path.join(str(cwd), "regions.tsv"), [n for n, _ in drafts], dmap, "-B" in argv)
    contigs, S, I, D = [], 0, 0, 0
    for (name, d), (_, o) in zip(drafts, outs):
        assert rebuilt[name] == o, f"{name}: the region dump does not rebuild the FASTA"
        us = []
        for b, e, t in units[name]:
            _, ops = ec.align_trimmed(d[b:e].encode(), t.encode())
            S, I, D = S + ops.count("X"), I + ops.count("I"), D + ops.count("D")
            us.append((b, e, t, ec.runs(ops)))
        contigs.append((name, len(d), ec.records(d, us)))
    assert vcf == ec.vcf_text(opt(argv, "-d"), contigs)
    assert (S, I, D) == tuple(int(x) for x in info[0][1:])
    # (4) -p 1: the same VCF
    if p1:
        a1 = list(argv)
        if "-p" in a1:
            a1[a1.index("-p") + 1] = "1"
        else:
            a1 += ["-p", "1"]
        run_(a1 + ["--vcf", "edits_p1.vcf"])
        assert open(os.path.join(str(cwd), "edits_p1.vcf")).read() == vcf
    return vcf, int(info[0][0])


@pytest.mark.parametrize("name", ["e2e_20k_s1", "e2e_200k_long_s3", "e2e_120k_ccs_s47"])
def test_vcf_goldens(name, tmp_path):
    man = eu.make_inputs(name, tmp_path)
    argv = shlex.split(man["command"])
    argv[0] = eu.BIN
    argv[argv.index("-t") + 1] = "16"
    vcf, n = check_vcf_run(argv, tmp_path, fasta_md5=man["expected_fasta_md5"])
    assert n > 0


@pytest.mark.parametrize("seed", sorted(eu.messy_seeds())[:2])
def test_vcf_messy_seeds(seed, tmp_path):
    spec = importlib.util.spec_from_file_location("gen_e2e", os.path.join(eu.GOLD, "gen_e2e.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    rec = eu.messy_seeds()[seed]
    argv, _, _ = gen.generate_messy(str(tmp_path), seed)
    argv = [eu.BIN] + list(argv)
    argv[argv.index("-t") + 1] = "8"                 # (as tests/test_gpu_e2e.py runs the messy seeds)
    check_vcf_run(argv, tmp_path, fasta_md5=rec["fasta_md5"])


def test_vcf_homopolymer_long_window(tmp_path):
    """the ~4 kbp poly-A LONG window of e2e_util.run_homopolymer_set: a unit the wide path aligns"""
    gen = eu.build_fast_generator()
    subprocess.check_output([gen, str(tmp_path), "141", "1", "90000", "9", "30", "150", "2000", "--bam", "--fast-hash", "--homopolymer", "29950", "4000", "--long", "25", "6000"])
    argv = [eu.BIN, "-d", "draft.fa", "-r", "reads.fa", "-s", "100k", "-c", "30", "-b", "sr.bam", "-B", "lr.bam", "-t", "16", "-i", "-o", "out.fa"]
    check_vcf_run(argv, tmp_path, p1=False)
    longest = max(int(r[2]) - int(r[1]) for r in (l.split("\t") for l in open(os.path.join(str(tmp_path), "regions.tsv"))) if r[3] == "LNG")
    assert longest > 3900


def test_vcf_shared_contig_three_contexts(tmp_path):
    """e2e_c4s_5m_s55 on three contexts of device 0 (contigs shared by contexts: piece mode), restarted from stage 1"""
    man, p, _, _ = eu.run_fast_case("e2e_c4s_5m_s55", tmp_path, threads=16, extra_args=["--devices", "0,0,0"], extra_env={"HYPO_ALLOW_DUP_DEVICES": "1"})
    assert eu.fasta_md5(tmp_path) == man["expected_fasta_md5"]
    argv = [eu.BIN] + man["command"].split()[1:]
    if "our_p" in man["args"] and "-p" in argv:
        argv[argv.index("-p") + 1] = str(man["args"]["our_p"])
    argv[argv.index("-t") + 1] = "16"
    if "-i" not in argv:
        argv += ["-i"]
    argv += ["--devices", "0,0,0"]
    assert os.path.exists(os.path.join(str(tmp_path), "aux", "stage.txt"))  # (the run above stored stage 1: the runs below restart from it)
    vcf, n = check_vcf_run(argv, tmp_path, env_extra={"HYPO_ALLOW_DUP_DEVICES": "1"}, fasta_md5=man["expected_fasta_md5"], p1=False)
    assert n > 0
