"""GPU: `hypo --guard-records` end to end against tests/guard_records_checker.py.

(a) Two goldens (e2e_20k_s1; the multi-contig -p 2 set e2e_5ctg_long_s21 at --qv-k 16, whose records hold clusters of 9 and 15
records, beyond the default limit of 8).  The unguarded run with --vcf --qv writes the golden's FASTA.  The --guard-records run's VCF
holds the same records; its FILTER column, its FASTA, the stdout line and the polished integers of its QV table are what the checker
computes; the PASS records applied to the draft give the FASTA; per contig the polished missing count is at most that of a plain
--kmer-guard run.  -p 1 writes the same three files and the flag alone the same FASTA.
(b) A forced partial acceptance on e2e_20k_s1, whose unguarded records at k = 21 form 183 clusters, 45 of them of 2..4 records (34 of
2, 8 of 3, 3 of 4; counted over the CPU stand-in of the device library with edit_checker.records and guard_checker.clusters).  The
reads are a tiling of T = the draft with the first record of every multi-record cluster and all records of the single-record
clusters applied: the by-record run reaches T's k-mers (polished missing count 0, clusters accepted in part), plain --kmer-guard can
only take or leave each cluster whole, so it is no better and writes another FASTA.
(c) --guard-records-max 2 on the same input: clusters of 3 or more records take the whole-cluster decision.
(d) No .tmp is left by any run."""
import hashlib
import os

import pytest

import edit_checker as ec
import guard_checker as gc
import guard_records_checker as grc
import qv_checker as qc
from test_gpu_guard import built, golden_argv, opt, run, three  # noqa: F401 (built: the module's autouse fixture)

pytestmark = pytest.mark.gpu


def check_by_record(cwd, argv, k, N, tag, p, records):
    """the --guard-records run `tag` (its three files and stdout) against the checker; records: those of the unguarded run.
    Returns (results per contig, table rows)."""
    path = lambda f: os.path.join(str(cwd), f)
    reads = opt(argv, "-r")
    R = qc.read_set([reads if reads.startswith("@") else path(reads)], k)
    drafts = [(n, qc.draft_text(s)) for n, s in ec.read_fastx(path(opt(argv, "-d")))]
    outs = ec.read_fastx(path("hypo_draft.fasta"))
    assert [n for n, _ in outs] == [n for n, _ in drafts]
    vcf = open(path(tag + ".vcf")).read()
    head, got_recs = ec.parse_vcf(vcf)
    _, got_filters = gc.parse_vcf_filters(vcf)
    assert got_recs == records, "the guarded VCF's records (FILTER aside) are not the unguarded run's"
    assert head.count(gc.FILTER_HEADER) == 1
    results = []
    for (name, D), (_, text) in zip(drafts, outs):
        recs = got_recs.get(name, [])
        res = grc.guard(D, recs, k, R, N)
        assert got_filters.get(name, []) == res.filters, name
        assert text == res.text, f"{name}: the FASTA record is not the draft with the accepted records applied"
        assert ec.apply([r for r, f in zip(recs, got_filters.get(name, [])) if f == "PASS"], D) == text
        results.append(res)
    lines = [l for l in p.stdout.splitlines() if "k-mer guard" in l]
    assert lines == [grc.info_line(k, N, results)]
    want = qc.rows(drafts, outs, k, R)
    assert open(path(tag + ".tsv")).read() == qc.table(want, k)
    for (name, dm, dt, pm, pt), res in zip(want, results):
        assert pm == dm + sum(a - r for r, a in res.scores) and pm <= dm, name      # clusters are independent
    return results, want


@pytest.mark.parametrize("name,k", [("e2e_20k_s1", None), ("e2e_5ctg_long_s21", 16)])
def test_guard_records_goldens(name, k, tmp_path):
    man, argv = golden_argv(name, tmp_path)
    kk = 21 if k is None else k
    kargs = [] if k is None else ["--qv-k", str(k)]
    files = lambda tag: ["--vcf", tag + ".vcf", "--qv", tag + ".tsv"] + kargs
    p0 = run(argv + files("u"), tmp_path)
    assert "Beginning from stage: 1" in p0.stdout and "k-mer guard" not in p0.stdout
    assert hashlib.md5(three(tmp_path, "u")[0]).hexdigest() == man["expected_fasta_md5"], "polished FASTA differs from the golden"
    _, records = ec.parse_vcf(open(os.path.join(str(tmp_path), "u.vcf")).read())
    p = run(argv + ["--guard-records"] + files("g"), tmp_path)
    results, want = check_by_record(tmp_path, argv, kk, 8, "g", p, records)
    sizes = [c[1] - c[0] for r in results for c in r.clusters]
    assert any(2 <= n <= 8 for n in sizes)
    if name == "e2e_5ctg_long_s21":
        assert opt(argv, "-p") == "2" and any(n > 8 for n in sizes)
    g = three(tmp_path, "g")
    # plain --kmer-guard: per contig its polished missing count is no smaller
    run(argv + ["--kmer-guard"] + files("w"), tmp_path)
    whole = qc.parse_table(open(os.path.join(str(tmp_path), "w.tsv")).read())
    for (name_, dm, dt, pm, pt), w in zip(want, whole):
        assert w[0] == name_ and pm <= w[4], name_
    # -p 1
    a1 = list(argv)
    if "-p" in a1:
        a1[a1.index("-p") + 1] = "1"
    else:
        a1 += ["-p", "1"]
    run(a1 + ["--guard-records"] + files("p1"), tmp_path)
    assert three(tmp_path, "p1") == g
    # the flag alone
    run(argv + ["--guard-records"] + kargs, tmp_path)
    assert open(os.path.join(str(tmp_path), "hypo_draft.fasta"), "rb").read() == g[0]
    assert sorted(f for f in os.listdir(str(tmp_path)) if f.endswith((".vcf", ".tsv", ".tmp"))) == ["g.tsv", "g.vcf", "p1.tsv", "p1.vcf", "u.tsv", "u.vcf", "w.tsv", "w.vcf"]


def test_guard_records_accepts_a_cluster_in_part(tmp_path):
    man, argv = golden_argv("e2e_20k_s1", tmp_path)
    k = 21
    drafts = [(n, qc.draft_text(s)) for n, s in ec.read_fastx(str(tmp_path / opt(argv, "-d")))]
    p0 = run(argv + ["--vcf", "u.vcf"], tmp_path)
    assert "Beginning from stage: 1" in p0.stdout
    _, records = ec.parse_vcf((tmp_path / "u.vcf").read_text())
    n_multi = 0
    with open(str(tmp_path / "tiles.fa"), "w") as f:
        for n, D in drafts:
            recs = records.get(n, [])
            cl = gc.clusters(recs, k)
            n_multi += sum(2 <= c[1] - c[0] <= 8 for c in cl)
            T = ec.apply([recs[c[0]] for c in cl], D)                 # the first record of every cluster (a single-record cluster's only one)
            tiles = [T[a:a + 150] for a in range(0, max(1, len(T) - 149), 50)] + [T[-150:]]
            f.write("".join(f">{n}_{i}\n{t}\n" for i, t in enumerate(tiles)))
    assert n_multi >= 1
    argv[argv.index("-r") + 1] = "tiles.fa"
    # the polish does not depend on -r from stage 1 on: the same records
    p = run(argv + ["--guard-records", "--vcf", "g.vcf", "--qv", "g.tsv"], tmp_path)
    results, want = check_by_record(tmp_path, argv, k, 8, "g", p, records)
    assert sum(r.rej_part for r in results) >= 1
    assert want[-1][3] == 0                                           # the guarded text: nothing missing
    g = three(tmp_path, "g")
    run(argv + ["--kmer-guard", "--vcf", "w.vcf", "--qv", "w.tsv"], tmp_path)
    w = three(tmp_path, "w")
    whole = qc.parse_table(w[2].decode())
    assert whole[-1][4] >= want[-1][3] and w[0] != g[0]
    # (c) --guard-records-max 2: clusters of 3 or more records are decided whole
    p2 = run(argv + ["--guard-records", "--guard-records-max", "2", "--vcf", "m.vcf", "--qv", "m.tsv"], tmp_path)
    assert "up to 2)" in p2.stdout
    results2, _ = check_by_record(tmp_path, argv, k, 2, "m", p2, records)
    big = [(r, i) for r in results2 for i, c in enumerate(r.clusters) if c[1] - c[0] >= 3]
    assert big and all(r.masks[i] is None and len({r.filters[j] for j in range(r.clusters[i][0], r.clusters[i][1])}) == 1 for r, i in big)
    assert not [f for f in os.listdir(str(tmp_path)) if f.endswith(".tmp")]
