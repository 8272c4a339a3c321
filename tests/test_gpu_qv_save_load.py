"""GPU: `hypo --qv-save / --qv-load` end to end, on vote_scenario() of tests/test_gpu_kmer_bridge_vote.py (e2e_20k_s1).  Every run
carries --qv --qv-bed --qv-spectra --kmer-guard --kmer-fix --kmer-bridge --kmer-bridge-vote 4 and writes the same file names, so
that two runs can be compared byte for byte: run A has those flags alone, run B also stores the set, run C loads what B stored.
B's and C's output files are A's, their stdout is A's but for the line about the file; the same again under --qv-min-count 2 and
valley, and from stage 0.  The stored file, parsed by the checker (tests/kset_file_checker.py), holds exactly the model's records of
the scenario's reads.  A file that is damaged, or of another k, ends the run with the file and the cause named and nothing left."""
import os
import subprocess

import pytest

import e2e_util as eu
import kset_file_checker as kf
import solid_checker as sc
from test_gpu_kmer_bridge_vote import vote_scenario
from test_gpu_qv import drop_aux, run
from test_gpu_qv_bed import stable

pytestmark = pytest.mark.gpu
K = 21
FLAGS = ["--qv", "q.tsv", "--qv-bed", "b.bed", "--qv-spectra", "s.spectra", "--kmer-guard", "--kmer-fix", "f.tsv", "--kmer-bridge", "br.tsv", "--kmer-bridge-vote", "4"]
FILES = ["q.tsv", "b.bed", "s.spectra", "f.tsv", "br.tsv"]
SAVED = "[Hypo::Hypo] Info: k-mer set saved to "
LOADED = "[Hypo::Hypo] Info: k-mer set loaded from "


class Runs:
    """the scenario in one directory, run A, and run B with the file it stored"""

    def __init__(self, tmp):
        if not os.path.exists(eu.BIN):
            eu.build_binary()
        self.tmp = tmp
        self.argv, self.out_path, self.reads = vote_scenario("e2e_20k_s1", tmp)
        self.a, self.a_files = self.go([])
        self.b, self.b_files = self.go(["--qv-save", "s.hks"])

    def path(self, f):
        return os.path.join(str(self.tmp), f)

    def go(self, extra):
        for f in FILES + [self.out_path]:
            if os.path.exists(self.path(f)):
                os.remove(self.path(f))
        p = run(self.argv + FLAGS + extra, self.tmp)
        files = {f: open(self.path(f), "rb").read() for f in FILES + [self.out_path]}
        assert all(files.values()) and self.no_tmp()
        return p, files

    def no_tmp(self):
        return not [f for f in os.listdir(str(self.tmp)) if f.endswith(".tmp")]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    return Runs(tmp_path_factory.mktemp("qv_save_load"))


def info(stdout, prefix):
    lines = [l for l in stdout.splitlines() if l.startswith(prefix)]
    assert len(lines) == 1, stdout[-1500:]
    return lines[0]


def test_save_changes_nothing_else(runs):
    assert runs.b_files == runs.a_files
    assert stable(runs.b.stdout, [SAVED]) == stable(runs.a.stdout) and len(stable(runs.b.stdout)) == len(stable(runs.a.stdout)) + 1
    assert SAVED not in runs.a.stdout and LOADED not in runs.a.stdout + runs.b.stdout
    m = kf.model(sc.parse_records([runs.reads]), K)
    line = info(runs.b.stdout, SAVED)
    size = os.path.getsize(runs.path("s.hks"))
    assert line.startswith(f"{SAVED}s.hks (k = {K}, {len(m)} distinct k-mers, {size} bytes, ") and line.endswith(" s)")
    # the line comes before any contig is polished
    assert runs.b.stdout.index(SAVED) < runs.b.stdout.index("BATCH-ID")


def test_the_file_holds_the_models_records(runs):
    m = kf.model(sc.parse_records([runs.reads]), K)
    k, n_keys, blocks, dig = kf.parse_file(runs.path("s.hks"))
    recs = [r for b in blocks for r in b]
    assert (k, n_keys) == (K, len(m)) and len(recs) == len(m)
    assert dict(recs) == m and dig == kf.digest(m)
    assert max(m.values()) > 30 and 1 in m.values()                       # every k-mer with its count, whatever a least count would say


@pytest.mark.parametrize("extra", [[], ["--qv-min-count", "2"], ["--qv-min-count", "valley"]])
def test_load_writes_what_the_build_writes(runs, extra):
    if extra:
        a, a_files = runs.go(extra)
    else:
        a, a_files = runs.a, runs.a_files
    c, c_files = runs.go(extra + ["--qv-load", "s.hks"])
    assert c_files == a_files
    assert stable(c.stdout, [LOADED]) == stable(a.stdout) and len(stable(c.stdout)) == len(stable(a.stdout)) + 1
    m = kf.model(sc.parse_records([runs.reads]), K)
    line = info(c.stdout, LOADED)
    assert line.startswith(f"{LOADED}s.hks (k = {K}, {len(m)} distinct k-mers, ") and line.endswith(" s)")
    assert c.stdout.index(LOADED) < c.stdout.index("BATCH-ID")
    # no read was parsed for the set (the run starts from stage 1: none was opened at all)
    assert "Beginning from stage: 1" in c.stdout
    assert "parsed for the QV alone" in a.stderr and "parsed for the QV alone" not in c.stderr and "no read parsed for it" in c.stderr
    if extra:
        assert "k-mer min count" in c.stdout and a_files != runs.a_files


def test_load_from_stage_0(runs, tmp_path):
    """the solid k-mers are counted from the reads, without the sink; the set comes from the file"""
    aux = runs.path("aux")
    os.rename(aux, str(tmp_path / "aux_kept"))
    try:
        a, a_files = runs.go([])
        assert "Beginning from stage: 0" in a.stdout and "the parse pass of the solid k-mers" in a.stderr
        drop_aux(runs.tmp)
        c, c_files = runs.go(["--qv-load", "s.hks"])
        assert "Beginning from stage: 0" in c.stdout and "the parse pass of the solid k-mers" not in c.stderr and "no read parsed for it" in c.stderr
        assert c_files == a_files
        assert stable(c.stdout, [LOADED]) == stable(a.stdout)
    finally:
        drop_aux(runs.tmp)
        os.rename(str(tmp_path / "aux_kept"), aux)


def damaged(runs, how):
    data = bytearray(open(runs.path("s.hks"), "rb").read())
    _, _, blocks, _ = kf.parse_bytes(bytes(data))
    n0 = len(blocks[0])
    if how == "truncated":
        return bytes(data[:len(data) - 10]), ["short read"]
    if how == "count":                                                    # another count, still 1..255: only the digest notices
        at = 24 + 8 + 8 * n0 + n0 // 2
        data[at] = data[at] % 255 + 1
        return bytes(data), ["digest mismatch"]
    at = 24 + 8 + 8 * (n0 // 3) + 7                                       # the top byte of a key
    data[at] |= 0x80
    return bytes(data), ["record %d" % (n0 // 3), "4^21"]


@pytest.mark.parametrize("how", ["truncated", "count", "key", "k"])
def test_refusals(runs, how):
    env = dict(os.environ, HYPO_REQUIRE_DEVICE="1")
    outs = ["r.fa", "r.qv", "r.bed", "r.spectra", "r.fix", "r.bridge"]
    flags = ["-o", "r.fa", "--qv", "r.qv", "--qv-bed", "r.bed", "--qv-spectra", "r.spectra", "--kmer-guard", "--kmer-fix", "r.fix", "--kmer-bridge", "r.bridge",
             "--kmer-bridge-vote", "4"]
    if how == "k":                                                        # a file of k = 31 for a run of --qv-k 21
        name = "s31.hks"
        run(runs.argv + ["-o", "r31.fa", "--qv-k", "31", "--qv-save", name], runs.tmp)
        assert kf.parse_file(runs.path(name))[0] == 31
        words = ["31", "21", "--qv-k"]
    else:
        name = "bad_%s.hks" % how
        data, words = damaged(runs, how)
        open(runs.path(name), "wb").write(data)
    p = subprocess.run(runs.argv + flags + ["--qv-load", name], cwd=str(runs.tmp), env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode != 0
    err = [l for l in p.stderr.splitlines() if l.startswith("[Hypo::QV] Error: --qv-load: ")]
    assert len(err) == 1 and name in err[0] and all(w in err[0] for w in words), p.stderr[-2000:]
    assert "BATCH-ID" not in p.stdout and LOADED not in p.stdout
    if how == "k":
        assert "Solid kmers" not in p.stdout                              # before any stage
    assert not [f for f in outs if os.path.exists(runs.path(f))] and runs.no_tmp()
