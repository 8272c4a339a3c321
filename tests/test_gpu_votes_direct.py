"""MI355X, straight through the C-ABI (ctypes): the kernels of support_kernel.hip against tests/votes_checker.py, a plain restatement
of the reference's two vote loops that tests/test_votes_checker_cpu.py pins to the C++ host loops on the same inputs.  The inputs
(tests/votes_cases.py) are tables and reads no genome generator produces: repeats that give a read k-mer several candidates, blocks
whose stretch of the tables outgrows the LDS tile of either block shape, gaps, every edge of a read's span, spans beyond 16 bits.
All four counter arrays are integers and deterministic (increments commute): every comparison is element for element, and every
case asserts — from its inputs and the checker, never from the device — that it reaches what it is there for."""
import ctypes as C

import numpy as np
import pytest

import votes_cases as cases
import votes_checker
from capi_util import ArmsReads, MegaWindows, ptr as _p
from hypo_amd import abi, capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return capi.HypoGpu(0).lib


def assert_same(what, got, want, pos):
    """element for element; a difference is reported with its first index, the position of that entry and both values"""
    assert got.shape == want.shape
    bad = np.nonzero(got != want)[0]
    if bad.size:
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} of {got.size} entries differ, the first at index {i} (position {int(pos[i])}): "
                             f"the device has {int(got[i])}, the checker {int(want[i])}")


def upload(lib, reads, read_contig, total_len):
    n = reads.rb.size
    cigar_off = np.arange(n + 1, dtype=np.uint32)
    cigar = ((reads.re - reads.rb).astype(np.uint32) << 4).astype(np.uint32)            # one M per read (the votes do not read it)
    A = ArmsReads(n, _p(reads.rb), _p(reads.re), _p(reads.qae), _p(reads.seq_off), _p(reads.reads2), reads.reads2.size, _p(cigar_off), _p(cigar), None)
    ctg = np.zeros(n, dtype=np.uint32) if read_contig is None else read_contig
    assert lib.hypo_gpu_reads_upload(C.byref(A), _p(ctg), C.c_uint64(total_len)) == abi.HYPO_OK, lib.hypo_gpu_last_error()


def device_kmer_votes(lib, c):
    upload(lib, c.reads, None, c.total_len)
    cov = np.full(c.spos.size, 0xDEAD, dtype=np.uint32); sup = np.full(c.spos.size, 0xDEAD, dtype=np.uint32)
    rc = lib.hypo_gpu_support_kmers(C.c_uint32(c.k), C.c_uint64(c.spos.size), _p(c.spos), _p(c.kids), _p(cov), _p(sup))
    assert rc == abi.HYPO_OK, lib.hypo_gpu_last_error()
    return cov, sup


def device_minimizer_votes(lib, c):
    upload(lib, c.reads, c.read_contig, c.total_len)
    T = c.tables
    n_ent = int(T.mw_off[T.n_info])
    W = MegaWindows(T.contig_base.size, _p(T.contig_base), _p(T.reg_base), _p(T.win_even), _p(T.info_base), _p(T.start), T.n_info, _p(T.mw_off), _p(T.rel_pos), _p(T.minimisers))
    cov = np.full(n_ent, 0xDEAD, dtype=np.uint32); sup = np.full(n_ent, 0xDEAD, dtype=np.uint32)
    assert lib.hypo_gpu_support_minimizers(C.byref(W), _p(cov), _p(sup)) == abi.HYPO_OK, lib.hypo_gpu_last_error()
    return cov, sup


@pytest.mark.parametrize("name", sorted(cases.KMER_CASES))
def test_kmer_votes_equal_the_checker(lib, name):
    """repeats_*: several candidates per read k-mer, the reverse visit order and the pvs_supp rule; range_ends: votes with the read
    k-mer exactly k in front of or behind its place in the contig; tags_*: the byte screen and the
    width of the ids; tiles256 / tiles64 / tiles64_plus_short: pause and resume at the end of a tile in either block shape; gaps:
    a stretch of more than three tiles no read touches; edges_k*: the ends of the coordinate space and of a read's span"""
    cases.kmer_condition(name)
    c = cases.kmer_case(name)
    want_cov, want_sup, _ = cases.kmer_expected(name)
    cov, sup = device_kmer_votes(lib, c)
    assert_same("coverage", cov, want_cov, c.spos)
    assert_same("support", sup, want_sup, c.spos)


def test_long_reads_vote_alike_through_both_block_shapes(lib):
    """the 64-lane shape (mean span above 1000) and the 256-lane shape (short reads appended behind the long ones until the mean is
    exactly 1000) leave the same counters on the entries the appended reads cannot touch"""
    a, b = cases.kmer_case("tiles64"), cases.kmer_case("tiles64_plus_short")
    assert cases.mean_span(a.reads) > cases.LONG_SPAN and cases.mean_span(b.reads) == cases.LONG_SPAN
    n = cases.n_original_entries(a)
    assert n > 9000 and (a.spos == b.spos).all() and (a.kids == b.kids).all()
    cov_a, sup_a = device_kmer_votes(lib, a)
    cov_b, sup_b = device_kmer_votes(lib, b)
    assert_same("coverage", cov_b[:n], cov_a[:n], a.spos)
    assert_same("support", sup_b[:n], sup_a[:n], a.spos)
    assert_same("support", sup_a, cases.kmer_expected("tiles64")[1], a.spos)


def test_a_small_call_after_a_large_one_sees_nothing_of_it(lib):
    """the work buffer of the context is reused: the counters of the second call are the checker's, whatever the first one left"""
    big, small = cases.kmer_case("tiles64_plus_short"), cases.kmer_case("edges_k15")
    assert big.spos.size > 40 * small.spos.size
    device_kmer_votes(lib, big)
    cov, sup = device_kmer_votes(lib, small)
    want_cov, want_sup, _ = cases.kmer_expected("edges_k15")
    assert_same("coverage", cov, want_cov, small.spos)
    assert_same("support", sup, want_sup, small.spos)
    mbig, msmall = cases.min_case("sixteen_bits_64"), cases.min_case("geometry")
    device_minimizer_votes(lib, mbig)
    cov, sup = device_minimizer_votes(lib, msmall)
    pos, _ = cases.entry_positions(msmall.tables)
    assert_same("minimizer coverage", cov, cases.min_expected("geometry")[0], pos)
    assert_same("minimizer support", sup, cases.min_expected("geometry")[1], pos)


def test_narrow_ids_of_a_kept_scan_vote_like_the_checker(lib):
    """support_kmers32 (32-bit ids, k <= 16) is reached through hypo_gpu_support_kmers_kept only: a repetitive contig scanned against
    a set that holds every 9-mer, reads whose blocks cross tiles, the checker on the positions and ids hypo_gpu_solid_scan reports"""
    k, handle = 9, 11
    codes, reads = cases.kept_contig_and_reads()
    n_bases = codes.size
    pad = np.concatenate([codes, np.zeros(n_bases % 2, np.uint8)]).reshape(-1, 2)
    p4 = ((pad[:, 0] << 4) | pad[:, 1]).astype(np.uint8)
    bits = np.full((1 << (2 * k)) // 64, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    assert lib.hypo_gpu_solid_set_upload(_p(bits), C.c_uint32(k)) == abi.HYPO_OK
    nw = (n_bases + 63) // 64
    words = np.zeros(nw, dtype=np.uint64); rank = np.zeros(nw + 1, dtype=np.uint64); kids = np.zeros(n_bases, dtype=np.uint64)
    ns = C.c_uint64(0)
    rc = lib.hypo_gpu_solid_scan(_p(p4), C.c_uint64(n_bases), C.c_uint32(k), _p(bits), _p(words), _p(kids), C.c_uint64(n_bases), _p(rank), C.byref(ns))
    assert rc == abi.HYPO_OK, lib.hypo_gpu_last_error()
    ns = int(ns.value)
    spos = np.nonzero(np.unpackbits(words.view(np.uint8), bitorder="little")[:n_bases])[0].astype(np.uint32)
    # (the scan's two homopolymer-edge tests leave a run of one base unmarked; the repeats of longer period are solid throughout)
    assert spos.size == ns and ns > 10_000
    case = cases.KmerCase("kept", k, n_bases + (n_bases & 1), spos, kids[:ns].copy(), reads)
    diag = {}
    want_cov, want_sup = votes_checker.kmer_votes(k, case.spos, case.kids, reads.rb, reads.re, reads.qae, reads.seq_off, reads.reads2, diag=diag)
    blocks = cases.kmer_blocks(case, 256)
    assert k <= 16 and cases.lanes_of(reads) == 256 and len(blocks) > 2 and all(bhi - blo > cases.KCAP for blo, bhi in blocks[:-1])
    assert diag["multi"] > 1000 and diag["refused"] > 1000, diag
    words2 = np.zeros(nw, dtype=np.uint64); rank2 = np.zeros(nw + 1, dtype=np.uint64); ns2 = C.c_uint64(0)
    rc = lib.hypo_gpu_solid_scan_keep(C.c_uint32(handle), _p(p4), C.c_uint64(n_bases), C.c_uint32(k), _p(words2), _p(rank2), C.byref(ns2))
    assert rc == abi.HYPO_OK, lib.hypo_gpu_last_error()
    try:
        assert ns2.value == ns and (words2 == words).all()
        upload(lib, reads, None, case.total_len)
        cov = np.full(ns, 0xDEAD, dtype=np.uint32); sup = np.full(ns, 0xDEAD, dtype=np.uint32)
        handles = np.array([handle], dtype=np.uint32); bases = np.array([0], dtype=np.uint32); tot = C.c_uint64(0)
        rc = lib.hypo_gpu_support_kmers_kept(C.c_uint32(k), C.c_uint32(1), _p(handles), _p(bases), _p(cov), _p(sup), C.byref(tot))
        assert rc == abi.HYPO_OK, lib.hypo_gpu_last_error()
        assert tot.value == ns
        assert_same("coverage", cov, want_cov, spos)
        assert_same("support", sup, want_sup, spos)
        # and the wide kernel on the same tables
        cov64, sup64 = device_kmer_votes(lib, case)
        assert_same("coverage (64-bit ids)", cov64, want_cov, spos)
        assert_same("support (64-bit ids)", sup64, want_sup, spos)
    finally:
        assert lib.hypo_gpu_solid_release(C.c_uint32(handle)) == abi.HYPO_OK


@pytest.mark.parametrize("name", sorted(cases.MIN_CASES))
def test_minimizer_votes_equal_the_checker(lib, name):
    """geometry: contigs at several bases, both parities of the mega-windows, reads on borders, inside strong regions, over several
    mega-windows, minimizers at the very ends of a read; ties: equal keys in a read's window, one minimizer many times in a
    mega-window; tiles256 / tiles64: an entry at every position, so a block's stretch outgrows its tile; sixteen_bits_*: a read that
    spans more than 65 535 bases, where the reference's 16-bit arithmetic wraps and the device must wrap with it; indels"""
    cases.min_condition(name)
    c = cases.min_case(name)
    want_cov, want_sup = cases.min_expected(name)
    cov, sup = device_minimizer_votes(lib, c)
    pos, _ = cases.entry_positions(c.tables)
    assert_same("coverage", cov, want_cov, pos)
    assert_same("support", sup, want_sup, pos)
