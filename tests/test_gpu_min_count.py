"""GPU: `hypo --qv-min-count` end to end.  With t = 2 and t = the valley, on a plain golden (k = 21) and a multi-contig -p 2 golden
(--qv-k 16), next to --vcf --qv --qv-bed and either guard: the FILTER column, the FASTA, the guard line, the QV table and the BED are
what the existing checkers (guard_checker, guard_records_checker, qv_checker, qv_track_checker) compute when they are handed
R_t = the read k-mers seen at least t times (tests/min_count_checker.py) in place of R; the min-count line on stdout is the checker's;
the PASS records applied to the draft give the FASTA; the draft lacks more k-mers than in the run without the flag.  --qv-min-count 1
is that run, byte for byte.  --qv-spectra writes the file it writes without the flag, and its valley is the threshold used here.  A
stage-0 run (one parse pass for the solid k-mers and the set) and a stage-1 run with the reads in 4 KiB chunks write the same files:
every window is counted once.  No .tmp is left by any run."""
import os

import pytest

import edit_checker as ec
import guard_checker as gc
import guard_records_checker as grc
import min_count_checker as mc
import qv_checker as qc
import qv_track_checker as tc
import spectra_checker as spc
from test_gpu_spectra import built, drop_aux, golden_argv, opt, run  # noqa: F401 (built: the module's autouse fixture)

pytestmark = pytest.mark.gpu
GOLDENS = [("e2e_20k_s1", None), ("e2e_5ctg_long_s21", 16)]
FILES = ("out.fa", "o.vcf", "o.qv", "o.bed")
OUTPUTS = ["--vcf", "o.vcf", "--qv", "o.qv", "--qv-bed", "o.bed"]


def kk(k):
    return (21, []) if k is None else (k, ["--qv-k", str(k)])


def stable(text):
    return sorted(l for l in text.splitlines() if not l.startswith("RESOURCES"))


def outputs(cwd):
    return {f: (cwd / f).read_bytes() for f in FILES}


def read_counts(cwd, argv, k):
    return mc.read_counts([os.path.join(str(cwd), opt(argv, "-r"))], k)


def check_run(cwd, argv, k, keys, counts, given, p, by_record):
    """the files and stdout of one run against the checkers with R_t.  Returns (t, the table's rows)."""
    path = lambda f: os.path.join(str(cwd), f)
    h = mc.histogram(counts)
    t = mc.threshold(h, given)
    Rt = mc.reliable_set(keys, counts, t)
    drafts = [(n, qc.draft_text(s)) for n, s in ec.read_fastx(path(opt(argv, "-d")))]
    outs = ec.read_fastx(path("out.fa"))
    assert [n for n, _ in outs] == [n for n, _ in drafts]
    vcf = open(path("o.vcf")).read()
    _, recs_of = ec.parse_vcf(vcf)
    _, filters_of = gc.parse_vcf_filters(vcf)
    results = []
    for (name, D), (_, text) in zip(drafts, outs):
        recs = recs_of.get(name, [])
        res = grc.guard(D, recs, k, Rt, 8) if by_record else gc.guard(D, recs, k, Rt)
        assert filters_of.get(name, []) == res.filters, name
        assert text == res.text, f"{name}: the FASTA record is not the draft with the accepted records applied"
        assert ec.apply([r for r, f in zip(recs, filters_of.get(name, [])) if f == "PASS"], D) == text
        results.append(res)
    assert [l for l in p.stdout.splitlines() if "k-mer guard" in l] == [grc.info_line(k, 8, results) if by_record else gc.info_line(k, results)]
    assert [l for l in p.stdout.splitlines() if "k-mer min count" in l] == [mc.info_line(k, h, given)]
    rows = qc.rows(drafts, outs, k, Rt)
    assert open(path("o.qv")).read() == qc.table(rows, k)
    bed = open(path("o.bed")).read()
    assert bed == tc.bed(outs, k, Rt)
    per_contig = {}
    for name, _, _, n in tc.parse_bed(bed):
        per_contig[name] = per_contig.get(name, 0) + n
    assert [per_contig.get(r[0], 0) for r in rows[:-1]] == [r[3] for r in rows[:-1]]        # the fourth column adds up to polished_missing
    return t, rows


@pytest.mark.parametrize("given", ["2", "valley"])
@pytest.mark.parametrize("name,k", GOLDENS)
def test_min_count_goldens(name, k, given, tmp_path):
    argv = golden_argv(name, tmp_path)
    k, kargs = kk(k)
    if name == "e2e_5ctg_long_s21":
        assert opt(argv, "-p") == "2"
    keys, counts = read_counts(tmp_path, argv, k)
    p0 = run(argv + OUTPUTS + ["--kmer-guard"] + kargs, tmp_path)
    assert "k-mer min count" not in p0.stdout
    off_table = (tmp_path / "o.qv").read_text()
    off = qc.parse_table(off_table)
    for by_record in (False, True):
        p = run(argv + OUTPUTS + ["--guard-records" if by_record else "--kmer-guard", "--qv-min-count", given] + kargs, tmp_path)
        assert "Beginning from stage: 1" in p.stdout
        t, rows = check_run(tmp_path, argv, k, keys, counts, given if given == "valley" else int(given), p, by_record)
        assert t >= 3 if given == "valley" else t == 2
        assert rows[-1][0] == "*" == off[-1][0] and rows[-1][2] == off[-1][2] and rows[-1][1] > off[-1][1]      # the same windows, more of them missing
        assert (tmp_path / "o.qv").read_text() != off_table


def test_one_is_the_run_without_the_flag(tmp_path):
    argv = golden_argv("e2e_20k_s1", tmp_path) + OUTPUTS + ["--guard-records"]
    p0 = run(argv, tmp_path)
    want = outputs(tmp_path)
    p = run(argv + ["--qv-min-count", "1"], tmp_path)
    assert outputs(tmp_path) == want
    assert stable(p.stdout) == stable(p0.stdout) and "min count" not in p.stdout


def test_spectra_keep_their_meaning(tmp_path):
    argv = golden_argv("e2e_20k_s1", tmp_path)
    run(argv + ["--qv", "plain.qv", "--qv-spectra", "plain.tsv"], tmp_path)
    text = (tmp_path / "plain.tsv").read_text()
    r = spc.parse_report(text)
    assert r["how"] == "valley"
    p = run(argv + ["--qv", "o.qv", "--qv-spectra", "o.tsv", "--qv-min-count", "valley"], tmp_path)
    assert (tmp_path / "o.tsv").read_text() == text                          # presence-based marks, the same counts
    line = [l for l in p.stdout.splitlines() if "k-mer min count" in l]
    keys, counts = read_counts(tmp_path, argv, 21)
    assert line == [mc.info_line(21, mc.histogram(counts), "valley")] and f">= {r['reliable_min']} (valley)" in line[0]
    assert f"reliable >= {r['reliable_min']})" in p.stdout                   # the same number twice
    assert f"{r['texts']['draft'][0]} of {r['reads_distinct']} read k-mers reliable" in line[0]
    # asm_only_windows is polished_missing of --qv without --qv-min-count
    plain, counted = qc.parse_table((tmp_path / "plain.qv").read_text())[-1], qc.parse_table((tmp_path / "o.qv").read_text())[-1]
    assert r["texts"]["polished"][3] == plain[4] < counted[4]
    # a given threshold, the guard beside it
    run(argv + ["--qv-spectra", "g0.tsv", "--kmer-guard"], tmp_path)
    run(argv + ["--qv-spectra", "g2.tsv", "--kmer-guard", "--qv-min-count", "2"], tmp_path)
    g0, g2 = spc.parse_report((tmp_path / "g0.tsv").read_text()), spc.parse_report((tmp_path / "g2.tsv").read_text())
    assert (g0["draft"] == g2["draft"]).all() and g0["texts"]["draft"] == g2["texts"]["draft"] and g0["reliable_min"] == g2["reliable_min"]
    assert (tmp_path / "g2.tsv").read_text() == spc.report_for([str(tmp_path / opt(argv, "-r"))], 21, [s for _, s in ec.read_fastx(str(tmp_path / opt(argv, "-d")))],
                                                                 [s for _, s in ec.read_fastx(str(tmp_path / "out.fa"))])


@pytest.mark.parametrize("name,k", GOLDENS)
def test_stage_0_and_small_chunks(name, k, tmp_path):
    argv = golden_argv(name, tmp_path) + OUTPUTS + ["--kmer-guard", "--qv-min-count", "valley"]
    k, kargs = kk(k)
    keys, counts = read_counts(tmp_path, argv, k)
    drop_aux(tmp_path)
    p = run(argv + kargs, tmp_path)
    assert "Beginning from stage: 0" in p.stdout and "the parse pass of the solid k-mers" in p.stderr
    check_run(tmp_path, argv, k, keys, counts, "valley", p, False)
    want = outputs(tmp_path)
    p1 = run(argv + kargs, tmp_path, {"HYPO_READ_CHUNK_KB": "4"})
    assert "Beginning from stage: 1" in p1.stdout and "reads parsed for the QV alone" in p1.stderr
    assert os.path.getsize(str(tmp_path / opt(argv, "-r"))) > 20 * 4096
    assert outputs(tmp_path) == want
    assert [l for l in p1.stdout.splitlines() if "k-mer min count" in l] == [l for l in p.stdout.splitlines() if "k-mer min count" in l]
