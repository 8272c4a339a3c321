"""MI355X, straight through the C-ABI (ctypes): what the reads, vote, arm and scan entry points of capi.hip refuse on the host, with
the return code and the text of hypo_gpu_last_error(), and one small hypo_gpu_arms_build_long + hypo_gpu_arms_download_long batch
against recorded results (tests/golden/capi_arms_long_small.json).  Every refusal here is made before anything is queued on the
device, so no kernel sees the bad arrays.  HYPO_GPU_LIB=<path> runs the module against another build of libhypo_gpu.so."""
import ctypes as C
import hashlib
import json
import os
import re

import numpy as np
import pytest

from hypo_amd import abi, capi, sim
from capi_util import ArmsReads, exact_reads, ptr as _p

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.environ.get("HYPO_GPU_LIB", capi.LIB_PATH)
GOLDEN = os.path.join(ROOT, "tests", "golden", "capi_arms_long_small.json")
U32 = C.c_uint32
U64 = C.c_uint64


class Regions(C.Structure):                        # HypoArmsRegions
    _fields_ = [("n_regions", U32), ("start", C.c_void_p), ("type", C.c_void_p), ("info", C.c_void_p), ("n_anchor_kmers", U64),
                ("anchor_kmers", C.c_void_p), ("k", U32), ("contig4", C.c_void_p)]


class Summary(C.Structure):                        # HypoArmsSummary
    _fields_ = [("n_windows", U32), ("n_arms", U32), ("arms2_bytes", U64), ("draft4_bytes", U64), ("out_bytes", U64)]


class Mega(C.Structure):                           # HypoMegaWindows
    _fields_ = [("n_contigs", U32), ("contig_base", C.c_void_p), ("reg_base", C.c_void_p), ("win_even", C.c_void_p), ("info_base", C.c_void_p),
                ("start", C.c_void_p), ("n_info", U32), ("mw_off", C.c_void_p), ("rel_pos", C.c_void_p), ("minimisers", C.c_void_p)]


def _u32(*v):
    return np.array(v, dtype=np.uint32)


def _fresh():
    """A library whose context holds nothing: hypo_gpu_init releases what an earlier test left (reads, batches, the k-mer set)."""
    return capi.HypoGpu(0, path=LIB).lib


def _refused(lib, rc, code, text):
    msg = lib.hypo_gpu_last_error().decode()
    assert rc == code and text in msg, (rc, msg)


CONTIG_LEN = 600
CODES, P4 = sim.random_contig(CONTIG_LEN, seed=21, n_frac=0.0)


class Reads:
    """A dozen 50-base exact-copy reads of the 600-base contig as HypoArmsReads; a test spoils its own copy."""

    def __init__(self):
        self.rb, self.re, self.qae, self.seq_off, self.reads2, self.cigar_off, self.cigar = exact_reads(CODES, 12, 50, np.random.default_rng(5))
        self.ctg = np.zeros(self.rb.size, dtype=np.uint32)
        self.file_rank = None

    @property
    def n(self):
        return self.rb.size

    def struct(self):
        return ArmsReads(self.n, _p(self.rb), _p(self.re), _p(self.qae), _p(self.seq_off), _p(self.reads2), self.reads2.size, _p(self.cigar_off),
                         _p(self.cigar), None if self.file_rank is None else _p(self.file_rank))

    def upload(self, lib, total_len=CONTIG_LEN):
        A = self.struct()
        return lib.hypo_gpu_reads_upload(C.byref(A), _p(self.ctg), U64(total_len))


# the per-record faults that hypo_gpu_reads_upload and hypo_gpu_arms_build (explicit reads) both refuse, as (spoil, message)
def _empty_span(r):
    r.re[1] = r.rb[1]


def _span_past_end(r):
    r.re[3] = CONTIG_LEN + 5


def _unsorted(r):
    r.rb[5] = r.rb[4] - 1


def _read_outside(r):
    r.seq_off[2] = r.reads2.size - 3


def _cigar_off_down(r):
    r.cigar_off[7] = r.cigar_off[6] - 1


RECORD_FAULTS = [(_empty_span, "alignment 1: span ["), (_span_past_end, "alignment 3: span ["),
                 (_unsorted, "alignments are not sorted by reference start (alignment 5)"), (_read_outside, "alignment 2: read outside reads2"),
                 (_cigar_off_down, "alignment 6: cigar_off decreases")]
FAULT_IDS = ["empty_span", "span_past_end", "unsorted", "read_outside_reads2", "cigar_off_decreases"]


def test_the_shared_reads_are_what_the_cases_below_assume():
    r = Reads()
    assert r.n == 12 and (np.diff(r.rb.astype(np.int64)) >= 0).all() and r.rb[4] >= 1 and r.re.max() <= CONTIG_LEN
    assert _fresh().hypo_gpu_abi_version() == abi.ABI_VERSION


# ---- hypo_gpu_reads_upload ---------------------------------------------------------------------------------------------------------
def test_reads_upload_null_probe_drops_the_resident_reads():
    lib = _fresh()
    assert Reads().upload(lib) == abi.HYPO_OK, lib.hypo_gpu_last_error()
    assert lib.hypo_gpu_support_kmers(U32(11), U64(0), None, None, None, None) == abi.HYPO_OK
    _refused(lib, lib.hypo_gpu_reads_upload(None, None, U64(0)), abi.HYPO_E_INVALID, "NULL argument")       # host/Hypo.cpp probes with this call
    _refused(lib, lib.hypo_gpu_support_kmers(U32(11), U64(0), None, None, None, None), abi.HYPO_E_INVALID, "no resident reads")
    r = Reads()
    A = r.struct()
    _refused(lib, lib.hypo_gpu_reads_upload(C.byref(A), None, U64(CONTIG_LEN)), abi.HYPO_E_INVALID, "NULL argument")
    A.qae = None
    _refused(lib, lib.hypo_gpu_reads_upload(C.byref(A), _p(r.ctg), U64(CONTIG_LEN)), abi.HYPO_E_INVALID, "NULL buffer in reads")


@pytest.mark.parametrize("spoil,text", RECORD_FAULTS, ids=FAULT_IDS)
def test_reads_upload_refuses_a_bad_record(spoil, text):
    lib = _fresh()
    r = Reads()
    spoil(r)
    _refused(lib, r.upload(lib), abi.HYPO_E_INVALID, text)
    _refused(lib, lib.hypo_gpu_support_kmers(U32(11), U64(0), None, None, None, None), abi.HYPO_E_INVALID, "no resident reads")


def test_reads_upload_refuses_a_contig_index_of_2_to_the_24():
    lib = _fresh()
    r = Reads()
    r.ctg[9] = 1 << 24
    _refused(lib, r.upload(lib), abi.HYPO_E_INVALID, "alignment 9: contig index 16777216 out of range")
    r.ctg[9] = (1 << 24) - 1                        # the largest index there is: accepted
    assert r.upload(lib) == abi.HYPO_OK, lib.hypo_gpu_last_error()


def test_reads_upload_reports_the_first_bad_record_and_its_first_fault():
    lib = _fresh()
    r = Reads()
    r.ctg[2] = 1 << 24
    _cigar_off_down(r)                              # record 6
    _empty_span(r)                                  # record 1, also spoiled twice: its span and its read
    r.seq_off[1] = r.reads2.size
    _refused(lib, r.upload(lib), abi.HYPO_E_INVALID, "alignment 1: span [")
    r = Reads()
    _cigar_off_down(r)                              # record 6 ...
    r.ctg[6] = 1 << 24                              # ... whose cigar_off is named before its contig
    r.re[10] = r.rb[10]
    _refused(lib, r.upload(lib), abi.HYPO_E_INVALID, "alignment 6: cigar_off decreases")


def test_reads_upload_reports_the_first_bad_record_across_its_eight_parts():
    """From 1 << 18 records on, eight threads check an eighth of the records each: the record named is still the first in record
    order, with its own fault, whichever part found it.  64 contigs of 4 096 reads, each contig a copy of the first."""
    lib = _fresh()
    L, T = 20_000, 64
    codes, _ = sim.random_contig(L, seed=6, n_frac=0.0)
    rb, re_, qae, seq_off, reads2, cigar_off, cigar = exact_reads(codes, 4096, 150, np.random.default_rng(6))
    m = rb.size
    assert m * T == 1 << 18
    r = Reads()
    copy = np.repeat(np.arange(T, dtype=np.uint64), m)
    r.rb, r.re, r.qae = np.tile(rb, T) + (copy * L).astype(np.uint32), np.tile(re_, T) + (copy * L).astype(np.uint32), np.tile(qae, T)
    r.seq_off, r.reads2 = np.tile(seq_off, T) + copy * np.uint64(reads2.size), np.tile(reads2, T)
    r.cigar_off, r.cigar, r.ctg = np.arange(m * T + 1, dtype=np.uint32), np.tile(cigar, T), copy.astype(np.uint32)
    assert r.upload(lib, total_len=L * T) == abi.HYPO_OK, lib.hypo_gpu_last_error()
    r.re[250_000] = r.rb[250_000]                   # part 7
    _refused(lib, r.upload(lib, total_len=L * T), abi.HYPO_E_INVALID, "alignment 250000: span [")
    r.cigar_off[200_001] = r.cigar_off[200_000] - 1                                # part 6, found by another thread than the one above
    _refused(lib, r.upload(lib, total_len=L * T), abi.HYPO_E_INVALID, "alignment 200000: cigar_off decreases")
    r.ctg[40_000] = 1 << 24                         # part 1
    _refused(lib, r.upload(lib, total_len=L * T), abi.HYPO_E_INVALID, "alignment 40000: contig index 16777216 out of range")
    r.seq_off[5] = r.reads2.size                    # part 0
    _refused(lib, r.upload(lib, total_len=L * T), abi.HYPO_E_INVALID, "alignment 5: read outside reads2")
    _refused(lib, lib.hypo_gpu_support_kmers(U32(11), U64(0), None, None, None, None), abi.HYPO_E_INVALID, "no resident reads")


# ---- hypo_gpu_arms_build / _long ---------------------------------------------------------------------------------------------------
def _region_types():
    """RegionType codes by name, read off the list in include/hypo_gpu.h."""
    text = open(os.path.join(ROOT, "include", "hypo_gpu.h")).read()
    names = re.search(r"RegionType \(include/globalDefs\.hpp:95-108\): ([A-Z ]+?) \*/", text).group(1).split()
    return {n: i for i, n in enumerate(names)}


class Plain:
    """Regions over the 600-base contig for hypo_gpu_arms_build: OTHER, SR, OTHER (+ the end marker)."""

    def __init__(self, start=(0, 250, 262, CONTIG_LEN), k=11, contig4=P4):
        t = _region_types()
        self.start = _u32(*start)
        self.type = np.array([t["OTHER"], t["SR"], t["OTHER"], t["SR"]], dtype=np.uint8)
        self.info = _u32(0, 1, 0, 0)
        self.anchors = np.zeros(3, dtype=np.uint64)
        self.contig4 = contig4
        self.k = k
        self.valid = np.zeros(3, dtype=np.uint8)
        self.sum = Summary()

    def build(self, lib, reads, long_mode=False):
        R = Regions(3, _p(self.start), _p(self.type), _p(self.info), self.anchors.size, _p(self.anchors), self.k, _p(self.contig4))
        A = reads.struct() if reads is not None else None
        f = lib.hypo_gpu_arms_build_long if long_mode else lib.hypo_gpu_arms_build
        return f(C.byref(R), C.byref(A) if A is not None else None, _p(self.valid), C.byref(self.sum))


def test_region_type_codes_are_the_headers():
    t = _region_types()
    assert len(t) == 12 and (t["OTHER"], t["LONG"], t["SR"], t["MSR"]) == (8, 9, 10, 11)


@pytest.mark.parametrize("spoil,text", RECORD_FAULTS, ids=FAULT_IDS)
def test_arms_build_refuses_a_bad_record(spoil, text):
    lib = _fresh()
    r = Reads()
    spoil(r)
    _refused(lib, Plain().build(lib, r), abi.HYPO_E_INVALID, text)


def test_arms_build_names_the_first_bad_record():
    lib = _fresh()
    r = Reads()
    _span_past_end(r)                               # record 3
    _cigar_off_down(r)                              # record 6
    _refused(lib, Plain().build(lib, r), abi.HYPO_E_INVALID, "alignment 3: span [")
    A = r.struct()
    A.cigar = None
    R = Plain()
    RS = Regions(3, _p(R.start), _p(R.type), _p(R.info), R.anchors.size, _p(R.anchors), R.k, _p(R.contig4))
    _refused(lib, lib.hypo_gpu_arms_build(C.byref(RS), C.byref(A), _p(R.valid), C.byref(R.sum)), abi.HYPO_E_INVALID, "NULL buffer in reads")


def test_arms_build_argument_checks():
    lib = _fresh()
    _refused(lib, Plain().build(lib, None), abi.HYPO_E_INVALID, "reads == NULL but no resident reads")
    _refused(lib, Plain().build(lib, None, long_mode=True), abi.HYPO_E_INVALID, "reads == NULL but no resident reads")
    _refused(lib, Plain(k=1).build(lib, Reads()), abi.HYPO_E_INVALID, "k=1 out of range 2..31")
    _refused(lib, Plain(k=32).build(lib, Reads()), abi.HYPO_E_INVALID, "k=32 out of range 2..31")
    _refused(lib, Plain(start=(0, 250, 250, CONTIG_LEN)).build(lib, Reads()), abi.HYPO_E_INVALID, "region 1 is empty or the starts are not increasing")
    # resident reads that were checked against another coordinate space; LONG windows never take the resident (short) reads
    assert Reads().upload(lib, total_len=CONTIG_LEN + 2) == abi.HYPO_OK, lib.hypo_gpu_last_error()
    _refused(lib, Plain().build(lib, None), abi.HYPO_E_INVALID, "the regions cover 600 bases, the resident reads were checked against 602")
    _refused(lib, Plain().build(lib, None, long_mode=True), abi.HYPO_E_INVALID, "reads == NULL but no resident reads")


def test_arms_build_leaves_one_huge_span_to_the_host():
    """One record over more than 16 384 bases and more than 64 x the mean span: HYPO_E_CAPACITY before anything is sent."""
    lib = _fresh()
    n, total = 100, 20_000
    r = Reads()
    r.rb = np.arange(n, dtype=np.uint32) * 10
    r.re = r.rb + 10
    r.re[0] = 17_000
    r.qae = np.full(n, 4, dtype=np.uint32)
    r.seq_off = np.zeros(n, dtype=np.uint64)
    r.reads2 = np.zeros(1, dtype=np.uint8)
    r.cigar_off = np.arange(n + 1, dtype=np.uint32)
    r.cigar = np.full(n, (4 << 4) | 0, dtype=np.uint32)
    R = Plain(start=(0, 250, 262, total), contig4=np.zeros(total // 2, dtype=np.uint8))
    _refused(lib, R.build(lib, r), abi.HYPO_E_CAPACITY, "an alignment spans 17000 reference bases, more than 64 x the mean span (179)")


# ---- the votes ---------------------------------------------------------------------------------------------------------------------
def test_support_kmers_argument_checks():
    lib = _fresh()
    assert Reads().upload(lib) == abi.HYPO_OK, lib.hypo_gpu_last_error()
    spos, kids, cov, sup = _u32(5, 9), np.zeros(2, dtype=np.uint64), _u32(0, 0), _u32(0, 0)
    _refused(lib, lib.hypo_gpu_support_kmers(U32(1), U64(2), _p(spos), _p(kids), _p(cov), _p(sup)), abi.HYPO_E_INVALID, "k=1 out of range 2..31")
    _refused(lib, lib.hypo_gpu_support_kmers(U32(32), U64(0), None, None, None, None), abi.HYPO_E_INVALID, "k=32 out of range 2..31")
    _refused(lib, lib.hypo_gpu_support_kmers(U32(11), U64(2), _p(spos), None, _p(cov), _p(sup)), abi.HYPO_E_INVALID, "NULL buffer")
    same = _u32(5, 5)
    _refused(lib, lib.hypo_gpu_support_kmers(U32(11), U64(2), _p(same), _p(kids), _p(cov), _p(sup)), abi.HYPO_E_INVALID, "solid positions are not increasing (entry 1)")
    assert lib.hypo_gpu_support_kmers(U32(11), U64(0), None, None, None, None) == abi.HYPO_OK


def test_support_kmers_kept_argument_checks():
    lib = _fresh()
    k, n_scan, handle = 11, 200, 3
    bits = sim.solid_bitset(CODES[:n_scan], k)
    assert lib.hypo_gpu_solid_set_upload(_p(bits), U32(k)) == abi.HYPO_OK
    nw = (n_scan + 63) // 64
    words, rank, ns = np.zeros(nw, dtype=np.uint64), np.zeros(nw + 1, dtype=np.uint64), U64(0)
    assert lib.hypo_gpu_solid_scan_keep(U32(handle), _p(P4), U64(n_scan), U32(k), _p(words), _p(rank), C.byref(ns)) == abi.HYPO_OK, lib.hypo_gpu_last_error()
    assert ns.value > 0
    assert Reads().upload(lib) == abi.HYPO_OK, lib.hypo_gpu_last_error()
    cov, sup, tot = np.zeros(2 * n_scan, dtype=np.uint32), np.zeros(2 * n_scan, dtype=np.uint32), U64(0)

    def kept(k_, handles, bases):
        return lib.hypo_gpu_support_kmers_kept(U32(k_), U32(handles.size), _p(handles), _p(bases), _p(cov), _p(sup), C.byref(tot))
    _refused(lib, kept(12, _u32(handle), _u32(0)), abi.HYPO_E_INVALID, "contig 0 was scanned with k = 11")
    _refused(lib, kept(1, _u32(handle), _u32(0)), abi.HYPO_E_INVALID, "k=1 out of range 2..31")
    _refused(lib, kept(k, _u32(handle), _u32(CONTIG_LEN - n_scan + 1)), abi.HYPO_E_INVALID, "contig 0 ends behind the 600 bases of the resident reads")
    _refused(lib, kept(k, _u32(handle, handle), _u32(0, n_scan - 1)), abi.HYPO_E_INVALID, "contig 1 overlaps the one before it")
    _refused(lib, kept(k, _u32(handle + 1), _u32(0)), abi.HYPO_E_INVALID, "contig 0: handle 4 holds no scan on this context")
    assert kept(k, _u32(handle, handle), _u32(0, n_scan)) == abi.HYPO_OK, lib.hypo_gpu_last_error()      # back to back is no overlap
    assert tot.value == 2 * ns.value


def test_support_minimizers_argument_checks():
    lib = _fresh()
    r = Reads()
    assert r.upload(lib) == abi.HYPO_OK, lib.hypo_gpu_last_error()
    cov, sup = np.zeros(4, dtype=np.uint32), np.zeros(4, dtype=np.uint32)
    t = dict(cb=_u32(0), rbase=_u32(0, 2), even=np.array([1], dtype=np.uint8), ib=_u32(0), start=_u32(0, CONTIG_LEN), n_info=1, mw_off=_u32(0, 1),
             rel=_u32(5, 5, 5, 5), mins=_u32(7, 7, 7, 7), nc=1)

    def vote(**kw):
        a = dict(t, **kw)
        W = Mega(a["nc"], _p(a["cb"]), _p(a["rbase"]), _p(a["even"]), _p(a["ib"]), _p(a["start"]), a["n_info"], _p(a["mw_off"]), _p(a["rel"]), _p(a["mins"]))
        return lib.hypo_gpu_support_minimizers(C.byref(W), _p(cov), _p(sup))
    _refused(lib, vote(rbase=_u32(0, 3, 2), nc=2, cb=_u32(0, 0), even=np.zeros(2, dtype=np.uint8), ib=_u32(0, 0), start=_u32(0, 300, CONTIG_LEN)), abi.HYPO_E_INVALID,
             "contig 1: reg_base decreases")
    _refused(lib, vote(start=_u32(CONTIG_LEN, CONTIG_LEN)), abi.HYPO_E_INVALID, "contig 0: region starts are not increasing")
    _refused(lib, vote(n_info=2, mw_off=_u32(0, 3, 2)), abi.HYPO_E_INVALID, "mw_off decreases at 1")
    _refused(lib, vote(ib=_u32(2)), abi.HYPO_E_INVALID, "contig 0: 2 region borders need MWMinimiserInfo entries up to 2, the tables hold 1")
    r.ctg[11] = 1                                   # a read of a second contig, tables of one
    assert r.upload(lib) == abi.HYPO_OK, lib.hypo_gpu_last_error()
    _refused(lib, vote(), abi.HYPO_E_INVALID, "the resident reads name contig 1, the tables hold 1 contigs")
    assert vote(mw_off=_u32(0, 0)) == abi.HYPO_OK   # no entries: nothing to vote on, nothing checked
    _refused(lib, lib.hypo_gpu_reads_upload(None, None, U64(0)), abi.HYPO_E_INVALID, "NULL argument")
    _refused(lib, vote(), abi.HYPO_E_INVALID, "no resident reads")


# ---- the scans ---------------------------------------------------------------------------------------------------------------------
def test_solid_scan_argument_checks():
    lib = _fresh()
    n = 200
    nw = (n + 63) // 64
    words, rank, kids, ns = np.zeros(nw, dtype=np.uint64), np.zeros(nw + 1, dtype=np.uint64), np.zeros(n, dtype=np.uint64), U64(0)

    def scan(k, bits=None):
        return lib.hypo_gpu_solid_scan(_p(P4), U64(n), U32(k), None if bits is None else _p(bits), _p(words), _p(kids), U64(n), _p(rank), C.byref(ns))

    def keep(k, handle=0):
        return lib.hypo_gpu_solid_scan_keep(U32(handle), _p(P4), U64(n), U32(k), _p(words), _p(rank), C.byref(ns))
    for k in (1, 32):
        _refused(lib, scan(k), abi.HYPO_E_INVALID, "k=%d out of range 2..31" % k)
        _refused(lib, keep(k), abi.HYPO_E_INVALID, "k=%d out of range 2..31" % k)
    _refused(lib, scan(11), abi.HYPO_E_INVALID, "bitset_words == NULL but no 11-mer set was uploaded")
    _refused(lib, keep(11), abi.HYPO_E_INVALID, "no 11-mer set was uploaded")
    bits = sim.solid_bitset(CODES[:n], 11)
    assert lib.hypo_gpu_solid_set_upload(_p(bits), U32(11)) == abi.HYPO_OK
    _refused(lib, scan(12), abi.HYPO_E_INVALID, "bitset_words == NULL but no 12-mer set was uploaded")
    _refused(lib, keep(12), abi.HYPO_E_INVALID, "no 12-mer set was uploaded")
    _refused(lib, keep(11, handle=1 << 24), abi.HYPO_E_INVALID, "handle or contig length out of range")
    _refused(lib, lib.hypo_gpu_solid_scan_keep(U32(0), None, U64(n), U32(11), _p(words), _p(rank), C.byref(ns)), abi.HYPO_E_INVALID, "NULL buffer")
    # the set on the device and the set handed over give the same scan, kept or not
    assert scan(11) == abi.HYPO_OK, lib.hypo_gpu_last_error()
    w1, r1, k1, n1 = words.copy(), rank.copy(), kids.copy(), ns.value
    assert n1 > 0
    assert scan(11, bits) == abi.HYPO_OK and ns.value == n1 and (words == w1).all() and (rank == r1).all() and (kids == k1).all()
    words[:] = 0
    rank[:] = 0
    assert keep(11, handle=7) == abi.HYPO_OK and ns.value == n1 and (words == w1).all() and (rank == r1).all()


# ---- resident batches --------------------------------------------------------------------------------------------------------------
def test_download_and_poa_before_any_build():
    lib = _fresh()
    sp = abi.ScoreParams(*abi.DEFAULT_SCORES)
    for suffix, text in (("", "no resident batch: call hypo_gpu_arms_build first"), ("_long", "no resident batch: call hypo_gpu_arms_build_long first")):
        _refused(lib, getattr(lib, "hypo_gpu_arms_download" + suffix)(None, None, None, None, None, None), abi.HYPO_E_INVALID, text)
        _refused(lib, getattr(lib, "hypo_gpu_arms_poa" + suffix)(C.byref(sp), None, None, None, None), abi.HYPO_E_INVALID, text)


# ---- hypo_gpu_arms_build_long + hypo_gpu_arms_download_long, accepted ---------------------------------------------------------------
def _long_batch(lib, codes, p4, reads, start, types, file_rank):
    """Builds the LONG batch of the pseudo regions and downloads it: (summary dict, region_valid, {array name: bytes})."""
    nr = len(types) - 1
    st, ty = _u32(*start), np.array(types, dtype=np.uint8)
    rb, re_, qae, seq_off, reads2, cigar_off, cigar = reads
    A = ArmsReads(rb.size, _p(rb), _p(re_), _p(qae), _p(seq_off), _p(reads2), reads2.size, _p(cigar_off), _p(cigar), None if file_rank is None else _p(file_rank))
    R = Regions(nr, _p(st), _p(ty), None, 0, None, 10, _p(p4))
    valid, s = np.full(nr, 9, dtype=np.uint8), Summary()
    assert lib.hypo_gpu_arms_build_long(C.byref(R), C.byref(A), _p(valid), C.byref(s)) == abi.HYPO_OK, lib.hypo_gpu_last_error()
    win = np.zeros(s.n_windows * C.sizeof(abi.Window), dtype=np.uint8)
    out = dict(windows=win, win_region=np.zeros(s.n_windows, dtype=np.uint32), arm_len=np.zeros(s.n_arms, dtype=np.uint32),
               arm_off=np.zeros(s.n_arms, dtype=np.uint64), arms2=np.zeros(s.arms2_bytes, dtype=np.uint8), draft4=np.zeros(s.draft4_bytes, dtype=np.uint8))
    rc = lib.hypo_gpu_arms_download_long(_p(out["windows"]), _p(out["win_region"]), _p(out["arm_len"]), _p(out["arm_off"]), _p(out["arms2"]), _p(out["draft4"]))
    assert rc == abi.HYPO_OK, lib.hypo_gpu_last_error()
    summary = dict(n_windows=s.n_windows, n_arms=s.n_arms, arms2_bytes=s.arms2_bytes, draft4_bytes=s.draft4_bytes, out_bytes=s.out_bytes)
    return summary, valid, {k: v.tobytes() for k, v in out.items()}


def test_arms_build_long_small_batch_equals_the_recorded_one():
    """Three LONG pseudo regions and one SR over a 3 000-base contig, 40 exact-copy reads of 150 bases.  The expected summary and the
    sha256 of every downloaded array are what this test computed (`got`, below) with the library of the commit before the entry
    points got their shared helpers."""
    lib = _fresh()
    t = _region_types()
    codes, p4 = sim.random_contig(3000, seed=33, n_frac=0.0)
    reads = exact_reads(codes, 40, 150, np.random.default_rng(8))
    start = (0, 1100, 1130, 2050, 3000)
    types = (t["LONG"], t["SR"], t["LONG"], t["LONG"], t["SR"])                   # (the last entry is the end marker)
    summary, valid, arrays = _long_batch(lib, codes, p4, reads, start, types, None)
    is_long = [int(x == t["LONG"]) for x in types[:-1]]
    assert summary["n_windows"] == sum(is_long) and valid.tolist() == is_long
    assert summary["n_arms"] > 0
    n = reads[0].size
    summary2, valid2, arrays2 = _long_batch(lib, codes, p4, reads, start, types, np.arange(n, dtype=np.uint32))
    assert summary2 == summary and valid2.tolist() == is_long and arrays2 == arrays
    got = dict(summary=summary, sha256={k: hashlib.sha256(v).hexdigest() for k, v in arrays.items()})
    assert got == json.load(open(GOLDEN))
    # ... and what was recorded is the contract's: the same arrays from the plain restatement of the host loops (tests/arms_checker.py)
    import arms_cases
    import arms_checker
    R = arms_cases.Regions(len(types) - 1, _u32(*start), np.array(types, dtype=np.uint8), None, 0, None, 10, p4, codes)
    A = arms_cases.Reads(reads[0], reads[1], reads[2], reads[3], reads[4], reads[4].size, reads[5], reads[6], None)
    x = arms_checker.build(R, A, long_mode=True)
    assert x.summary == summary and x.region_valid == is_long
    assert {k: v.tobytes() for k, v in arms_cases.as_arrays(x).items()} == arrays
