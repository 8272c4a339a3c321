"""GPU: `hypo --kmer-guard` end to end against tests/guard_checker.py.

(a) Three goldens (a plain set, a -B set, a multi-contig -p 2 set).  The unguarded run with --vcf --qv writes the golden's FASTA.
The guarded run's VCF holds the same records; its FILTER column, its FASTA, the stdout counts and the polished integers of its QV
table are what the checker computes from the draft, the unguarded records, the reads and k; the PASS records applied to the draft
give the FASTA; the polished missing count is at most the draft's and at most the unguarded run's.  -p 1 writes the same three
files and the guard alone the same FASTA.  Then aux/ is dropped: a stage-0 run (one parse pass for the solid k-mers and the set) is
checked against the checker from its own records, writes the three files of the stage-1 run whenever its polish is that run's (the
solid set it derives from the reads need not be the one the golden came with), and a stage-1 run over the set it stored (the reads
parsed for the k-mer set alone) writes the same three files again.
(b) e2e_20k_s1 with its own aux/ and, as -r, a tiling of the draft itself: every draft k-mer is in R, so a cluster survives only
if it adds no k-mer the draft lacks; at least one record is rejected and the table's polished missing count is 0.
(c) No .tmp is left by any run."""
import hashlib
import os
import shlex
import shutil
import subprocess

import pytest

import e2e_util as eu
import edit_checker as ec
import guard_checker as gc
import qv_checker as qc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(eu.BIN):
        eu.build_binary()


def run(argv, cwd):
    env = dict(os.environ, HYPO_REQUIRE_DEVICE="1")
    p = subprocess.run(argv, cwd=str(cwd), env=env, capture_output=True, text=True, timeout=1800)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert not [f for f in os.listdir(str(cwd)) if f.endswith(".tmp")]
    return p


def opt(argv, flag, default=None):
    return argv[argv.index(flag) + 1] if flag in argv else default


def golden_argv(name, tmp_path):
    man = eu.make_inputs(name, tmp_path)
    argv = shlex.split(man["command"])
    argv[0] = eu.BIN
    argv[argv.index("-t") + 1] = "16"
    assert "-i" in argv and "-o" not in argv
    return man, argv


def three(cwd, tag):
    return [open(os.path.join(str(cwd), f), "rb").read() for f in ("hypo_draft.fasta", tag + ".vcf", tag + ".tsv")]


def check_guarded(cwd, argv, k, tag, p, records=None):
    """the guarded run `tag` (its three files and stdout) against the checker; records: {contig: [(pos, ref, alt, info)]} of the
    unguarded run (None: the guarded VCF's own).  Returns (results per contig, table rows)."""
    path = lambda f: os.path.join(str(cwd), f)
    reads = opt(argv, "-r")
    R = qc.read_set([reads if reads.startswith("@") else path(reads)], k)
    drafts = [(n, qc.draft_text(s)) for n, s in ec.read_fastx(path(opt(argv, "-d")))]
    outs = ec.read_fastx(path("hypo_draft.fasta"))
    assert [n for n, _ in outs] == [n for n, _ in drafts]
    vcf = open(path(tag + ".vcf")).read()
    head, got_recs = ec.parse_vcf(vcf)
    _, got_filters = gc.parse_vcf_filters(vcf)
    if records is not None:
        assert got_recs == records, "the guarded VCF's records (FILTER aside) are not the unguarded run's"
    assert head.count(gc.FILTER_HEADER) == 1 and head.index(gc.FILTER_HEADER) == len(head) - 2 and head[-3].startswith("##INFO=")
    results = []
    for (name, D), (_, text) in zip(drafts, outs):
        recs = got_recs.get(name, [])
        res = gc.guard(D, recs, k, R)
        assert got_filters.get(name, []) == res.filters, name
        assert text == res.text, f"{name}: the FASTA record is not the draft with the accepted records applied"
        assert ec.apply([r for r, f in zip(recs, got_filters.get(name, [])) if f == "PASS"], D) == text
        results.append(res)
    lines = [l for l in p.stdout.splitlines() if "k-mer guard" in l]
    assert lines == [gc.info_line(k, results)]
    want = qc.rows(drafts, outs, k, R)
    table = open(path(tag + ".tsv")).read()
    assert table == qc.table(want, k)
    for (name, dm, dt, pm, pt), (_, D), res in zip(want, drafts, results):
        accepted = sum(a - r for (r, a) in res.scores if a <= r)
        assert pm == dm + accepted and pm <= dm, name                  # missing(final) = missing(D) + the accepted clusters' changes
    return results, want


@pytest.mark.parametrize("name,k", [("e2e_20k_s1", None), ("e2e_200k_long_s3", None), ("e2e_5ctg_long_s21", 16)])
def test_guard_goldens(name, k, tmp_path):
    man, argv = golden_argv(name, tmp_path)
    if name == "e2e_5ctg_long_s21":
        assert opt(argv, "-p") == "2"
    if name == "e2e_200k_long_s3":
        assert "-B" in argv
    kk = 21 if k is None else k
    kargs = [] if k is None else ["--qv-k", str(k)]
    files = lambda tag: ["--vcf", tag + ".vcf", "--qv", tag + ".tsv"] + kargs
    # unguarded, from stage 1 over the golden's own aux/
    p0 = run(argv + files("u"), tmp_path)
    assert "Beginning from stage: 1" in p0.stdout and "k-mer guard" not in p0.stdout
    assert hashlib.md5(three(tmp_path, "u")[0]).hexdigest() == man["expected_fasta_md5"], "polished FASTA differs from the golden"
    _, records = ec.parse_vcf(open(os.path.join(str(tmp_path), "u.vcf")).read())
    unguarded = qc.parse_table(open(os.path.join(str(tmp_path), "u.tsv")).read())
    # guarded
    p = run(argv + ["--kmer-guard"] + files("g"), tmp_path)
    assert "Beginning from stage: 1" in p.stdout
    results, want = check_guarded(tmp_path, argv, kk, "g", p, records)
    assert sum(r.n_clusters for r in results) > 0
    for (name_, dm, dt, pm, pt), u in zip(want, unguarded):
        assert u[0] == name_ and (u[1], u[2]) == (dm, dt) and pm <= dm and pm <= u[4], name_
    g = three(tmp_path, "g")
    # -p 1
    a1 = list(argv)
    if "-p" in a1:
        a1[a1.index("-p") + 1] = "1"
    else:
        a1 += ["-p", "1"]
    run(a1 + ["--kmer-guard"] + files("p1"), tmp_path)
    assert three(tmp_path, "p1") == g
    # the guard alone
    run(argv + ["--kmer-guard"] + kargs, tmp_path)
    assert open(os.path.join(str(tmp_path), "hypo_draft.fasta"), "rb").read() == g[0]
    assert sorted(f for f in os.listdir(str(tmp_path)) if f.endswith((".vcf", ".tsv"))) == ["g.tsv", "g.vcf", "p1.tsv", "p1.vcf", "u.tsv", "u.vcf"]
    # stage 0: one parse pass for the solid k-mers and the k-mer set
    shutil.rmtree(os.path.join(str(tmp_path), "aux"))
    ps = run(argv + ["--kmer-guard"] + files("s0"), tmp_path)
    assert "Beginning from stage: 0" in ps.stdout and "the parse pass of the solid k-mers" in ps.stderr
    check_guarded(tmp_path, argv, kk, "s0", ps)
    s0 = three(tmp_path, "s0")
    if ec.parse_vcf(s0[1].decode())[1] == records:                   # the same polish: the same three files
        assert s0 == g
    p1 = run(argv + ["--kmer-guard"] + files("s1"), tmp_path)
    assert "Beginning from stage: 1" in p1.stdout and "reads parsed for the QV alone" in p1.stderr
    assert three(tmp_path, "s1") == s0


def test_guard_rejects_what_the_reads_do_not_hold(tmp_path):
    man, argv = golden_argv("e2e_20k_s1", tmp_path)
    k = 21
    drafts = [(n, qc.draft_text(s)) for n, s in ec.read_fastx(str(tmp_path / opt(argv, "-d")))]
    with open(str(tmp_path / "tiles.fa"), "w") as f:
        for n, D in drafts:
            tiles = [D[a:a + 150] for a in range(0, max(1, len(D) - 149), 50)] + [D[-150:]]
            f.write("".join(f">{n}_{i}\n{t}\n" for i, t in enumerate(tiles)))
    argv[argv.index("-r") + 1] = "tiles.fa"
    R = qc.read_set([str(tmp_path / "tiles.fa")], k)
    assert all(qc.seq_stats(D, k, R)[1] == 0 for _, D in drafts)     # every window of the draft is in R
    p0 = run(argv + ["--vcf", "u.vcf"], tmp_path)
    assert "Beginning from stage: 1" in p0.stdout
    assert eu.fasta_md5(tmp_path) == man["expected_fasta_md5"]
    _, records = ec.parse_vcf((tmp_path / "u.vcf").read_text())
    p = run(argv + ["--kmer-guard", "--vcf", "g.vcf", "--qv", "g.tsv"], tmp_path)
    results, want = check_guarded(tmp_path, argv, k, "g", p, records)
    assert all(r == 0 for res in results for r, _ in res.scores)
    assert want[-1][1] == 0 and want[-1][3] == 0                      # draft and guarded text: nothing missing
    filters = [f for res in results for f in res.filters]
    assert filters.count("kmer") >= 1
    assert eu.fasta_md5(tmp_path) != man["expected_fasta_md5"]
