"""GPU: `hypo --kmer-bridge --kmer-bridge-vote` end to end, on planted_scenario() of tests/test_gpu_kmer_bridge.py with a few reads
appended to the reads file (vote_scenario): the scenario's own read errors already give sites whose second walk is seen once, for
two planted sites the appended reads carry a base between the anchors another way twelve times, about half of what the reads over
it say, so that those sites stay too close to call, and for three more sites they carry it another way twice, so that
those sites are ambiguous under --qv-min-count 2 as well and the vote chooses there (about 25 against 2).  The run without a flag gives the base FASTA, the run with
--kmer-bridge alone the base of the comparison; with the vote the FASTA, the TSV and both Info lines are the checker's
(tests/kmer_vote_checker.py) over the base FASTA, the TSV applied backwards gives the base FASTA, the bridges that needed no vote are
those of the run without it, a contig's missing k-mers drop by exactly the sum of the file's counts, and no .tmp is left.  Then next
to --kmer-fix, --qv and --qv-bed, and next to --qv-spectra.

The floors are those the checker alone meets on the CPU stand-in's base FASTA of this scenario (DESIGN.md "k-mer bridge vote" has
the table): at least 3 chosen sites and at least one too close, at t = 1 and under --qv-min-count 2."""
import os
import re

import pytest

import e2e_util as eu
import edit_checker as ec
import kmer_bridge_checker as kb
import kmer_fix_checker as fc
import kmer_vote_checker as kv
import qv_checker as qc
import qv_track_checker as tc
from test_gpu_kmer_bridge import INFO, apply_backwards, planted_scenario
from test_gpu_kmer_fix import fasta_bytes
from test_gpu_qv import opt, run
from test_gpu_qv_bed import stable

pytestmark = pytest.mark.gpu
RATIO = 4
CLOSE_COPIES, CLOSE_SITES, PICK_K = 12, 2, 31                             # (what lies between the anchors at k = 31 does at k = 21)
TWICE_COPIES, TWICE_SITES = 2, 3


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(eu.BIN):
        eu.build_binary()


def second_walks(draft, reads_path, n_sites):
    """reads that give a site a second walk: for the last n_sites sites of the draft (where no alignment reaches) whose one walk (at
    k = PICK_K, in the reads as they are) has bases between the two anchors (a planted deletion or pair of substitutions), the left
    anchor and the walk with the middle one of those bases changed into a base that neither the walk nor the draft has there, 40
    bases of the draft on either side; the sites taken are at least 300 bases apart"""
    R = qc.read_set([reads_path], PICK_K)
    Rs = kb.as_set(R)
    out = []
    for name, s in draft:
        S = s.upper().encode()
        last = len(S) + 300
        for start, end, n, a, b, d0 in reversed(kb.sites(S, PICK_K, R)[0]):
            st, steps, w = kb.search(S[a:a + PICK_K], S[b:b + PICK_K], max(1, d0 - kb.DEFAULT_SLACK), d0 + kb.DEFAULT_SLACK, kb.BUDGET, PICK_K, Rs)
            if st != kb.UNIQUE or len(w) <= PICK_K or a < 40 or b + PICK_K + 40 > len(S) or a + 300 > last:
                continue                                                   # (300 bases from the site taken before: a read of one holds no base of the other)
            last = a
            old, new = S[a:b + PICK_K], S[a:a + PICK_K] + w
            q = PICK_K + (len(w) - PICK_K) // 2                            # new[PICK_K:len(w)] lies between the anchors
            base = next(c for c in b"ACGT" if c != new[q] and c != old[min(q, len(old) - 1)])
            alt = new[:q] + bytes([base]) + new[q + 1:]
            out.append((S[a - 40:a] + alt + S[b + PICK_K:b + PICK_K + 40]).decode())
            if len(out) == n_sites:
                return out
    return out


def vote_scenario(name, tmp_path):
    argv, out_path, reads = planted_scenario(name, tmp_path)
    extra = second_walks(ec.read_fastx(os.path.join(str(tmp_path), opt(argv, "-d"))), reads, CLOSE_SITES + TWICE_SITES)
    assert len(extra) == CLOSE_SITES + TWICE_SITES
    with open(reads, "a") as f:
        for i, r in enumerate(extra):                                      # the first CLOSE_SITES of them often, the others twice
            for j in range(CLOSE_COPIES if i < CLOSE_SITES else TWICE_COPIES):
                f.write(f">second{i}_{j}\n{r}\n")
    return argv, out_path, reads


def check_vote_pair(base_fa, new_fa, tsv_path, k, C, t, stdout=None, tsv_name=None, ratio=RATIO):
    """the new FASTA, the TSV and the Info lines against the checker run on the base FASTA; returns (rows of the TSV, Stats, Vote)"""
    base = ec.read_fastx(base_fa)
    want, want_tsv, st, vt = kv.run(base, k, C, t, ratio)
    assert open(new_fa, "rb").read() == fasta_bytes(want), "the FASTA is not the checker's"
    text = open(tsv_path).read()
    assert text == want_tsv
    rows = kv.parse_tsv(text)
    new = ec.read_fastx(new_fa)
    assert fasta_bytes(apply_backwards(new, [r[:6] for r in rows])) == fasta_bytes(base)
    assert [r[0] for r in rows] == sorted((r[0] for r in rows), key=[n for n, _ in base].index)          # contigs in draft order
    for r in rows:
        assert (r[6] == 1 and r[7] == ".") or (2 <= r[6] <= kv.W and re.fullmatch(r"\d+/\d+", r[7])), r
    assert st.bridged == len(rows) and vt.chosen == sum(1 for r in rows if r[6] > 1) and st.ambiguous == vt.asked - vt.chosen
    # the identity: a contig's missing k-mers drop by the sum of its lines' counts
    R = kv.reliable(C, t)[0]
    for (name, s0), (_, s1) in zip(base, new):
        assert qc.seq_stats(s1, k, R)[1] == qc.seq_stats(s0, k, R)[1] - sum(r[4] for r in rows if r[0] == name), name
    if stdout is not None:
        assert re.findall(INFO, stdout, flags=re.M) == kv.info_lines(tsv_name, k, kb.DEFAULT_MAX, kb.DEFAULT_SLACK, ratio, st, vt)
    return rows, st, vt


@pytest.mark.parametrize("k,t", [(None, 1), (31, 1), (None, 2)])
def test_vote_pair(k, t, tmp_path):
    argv, out_path, reads = vote_scenario("e2e_20k_s1", tmp_path)
    kk = 21 if k is None else k
    kargs = ([] if k is None else ["--qv-k", str(k)]) + ([] if t == 1 else ["--qv-min-count", str(t)])
    C = kv.read_count_map([reads], kk)
    path = lambda f: str(tmp_path / f)
    no_tmp = lambda: not [f for f in os.listdir(str(tmp_path)) if f.endswith(".tmp")]
    run(argv + ["-o", "base.fa"], tmp_path)
    p0 = run(argv + ["-o", "b.fa", "--kmer-bridge", "b.tsv"] + kargs, tmp_path)
    assert "k-mer bridge vote" not in p0.stdout
    p = run(argv + ["--kmer-bridge", "v.tsv", "--kmer-bridge-vote", str(RATIO)] + kargs, tmp_path)
    rows, st, vt = check_vote_pair(path("base.fa"), out_path, path("v.tsv"), kk, C, t, p.stdout, "v.tsv")
    assert no_tmp()
    # the run without the vote: its file is byte for byte the checker's without the two columns, its bridges are the vote's that needed none
    want0, tsv0, st0 = kb.run(ec.read_fastx(path("base.fa")), kk, kv.reliable(C, t)[0])
    assert open(path("b.tsv")).read() == tsv0 and open(path("b.fa"), "rb").read() == fasta_bytes(want0)
    assert [r[:5] for r in kb.parse_tsv(tsv0)] == [r[:5] for r in rows if r[6] == 1]
    assert st0.ambiguous == vt.asked and st.bridged == st0.bridged + vt.chosen and (st.intervals, st.sites, st.over_budget) == (st0.intervals, st0.sites, st0.over_budget)
    # stdout: the lines of the run without the vote, and one more
    bridge = ["[Hypo::Hypo] Info: k-mer bridge "]
    assert stable(p.stdout, bridge) == stable(p0.stdout, bridge)
    assert len(stable(p.stdout)) == len(stable(p0.stdout)) + 1
    # the floors (the checker's, on the CPU stand-in's base FASTA)
    assert vt.close >= 1 and vt.chosen >= 3, vt.tuple()
    # another ratio: the checker's again
    p = run(argv + ["-o", "r.fa", "--kmer-bridge", "r.tsv", "--kmer-bridge-vote", "2"] + kargs, tmp_path)
    rows2, st2, vt2 = check_vote_pair(path("base.fa"), path("r.fa"), path("r.tsv"), kk, C, t, p.stdout, "r.tsv", ratio=2)
    assert vt2.asked == vt.asked and vt2.chosen >= vt.chosen >= 3
    assert no_tmp()


def test_vote_with_the_other_flags(tmp_path):
    argv, out_path, reads = vote_scenario("e2e_20k_s1", tmp_path)
    k = 21
    R = qc.read_set([reads], k)
    C = kv.read_count_map([reads], k)
    path = lambda f: str(tmp_path / f)
    run(argv + ["-o", "base.fa"], tmp_path)
    vote = ["--kmer-bridge-vote", str(RATIO)]
    p = run(argv + ["-o", "new.fa", "--kmer-fix", "f.tsv", "--qv", "q.tsv", "--qv-bed", "b.bed", "--kmer-bridge", "v.tsv"] + vote, tmp_path)
    # the fixes over the base text, the bridges and the vote over the fixed text, both files their checkers'
    fixed, fix_tsv, fix_st = fc.run(ec.read_fastx(path("base.fa")), k, R)
    open(path("fixed_by_checker.fa"), "wb").write(fasta_bytes(fixed))
    assert open(path("f.tsv")).read() == fix_tsv
    rows, st, vt = check_vote_pair(path("fixed_by_checker.fa"), path("new.fa"), path("v.tsv"), k, C, 1, p.stdout, "v.tsv")
    assert vt.chosen >= 1 and vt.close >= 1
    # --qv and --qv-bed describe the final text
    new = ec.read_fastx(path("new.fa"))
    t1 = qc.parse_table(open(path("q.tsv")).read())
    assert [(r[0], r[4], r[5]) for r in t1[:-1]] == [(n, m, t) for n, (t, m) in ((n, qc.seq_stats(s, k, R)) for n, s in new)]
    assert open(path("b.bed")).read() == tc.bed(new, k, R)
    # next to --qv-spectra the set counts in the spectra's planes: the same files
    run(argv + ["-o", "s.fa", "--qv-spectra", "s.spectra", "--kmer-fix", "sf.tsv", "--kmer-bridge", "s.tsv"] + vote, tmp_path)
    assert open(path("s.tsv")).read() == open(path("v.tsv")).read() and open(path("s.fa"), "rb").read() == open(path("new.fa"), "rb").read()
    assert not [f for f in os.listdir(str(tmp_path)) if f.endswith(".tmp")]
