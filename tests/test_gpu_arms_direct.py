"""MI355X, straight through the C-ABI (ctypes): the kernels of arms_kernel.hip against tests/arms_checker.py, a plain restatement of the
host loops of arm selection that tests/test_arms_checker_cpu.py pins to the C++ host mirror on the same inputs.  The inputs
(tests/arms_cases.py) are region tables and reads no genome generator produces: CIGAR operations that end on a border, every outcome
of the four anchor searches, both sides of every pruning threshold, a file order far from the position order, every packing offset,
prefix sums over more than 1024 and more than 1024 x 1024 items.  Everything is integers and bytes: every comparison is element for
element, and every case asserts — from its inputs and the checker, never from the device — that it reaches what it is there for.
HYPO_GPU_LIB=<path> runs the module against another build of libhypo_gpu.so."""
import ctypes as C
import os

import numpy as np
import pytest

import arms_cases as cases
from capi_util import ArmsReads, ArmsRegions, ArmsSummary, ptr as _p
from hypo_amd import abi, capi

pytestmark = pytest.mark.gpu

LIB = os.environ.get("HYPO_GPU_LIB", capi.LIB_PATH)
FIELDS = ("windows", "win_region", "arm_len", "arm_off", "arms2", "draft4")


@pytest.fixture(scope="module")
def gpu():
    return capi.HypoGpu(0, path=LIB)


@pytest.fixture(scope="module")
def lib(gpu):
    return gpu.lib


def reads_struct(A):
    return ArmsReads(A.rb.size, _p(A.rb), _p(A.re), _p(A.qae), _p(A.seq_off), _p(A.reads2), A.reads2_bytes, _p(A.cigar_off), _p(A.cigar),
                     None if A.file_rank is None else _p(A.file_rank))


def build(lib, c, resident=False):
    """hypo_gpu_arms_build / _build_long of the case: (region_valid, summary as a dict)"""
    cases.check_tables(c)
    R = c.regions
    RS = ArmsRegions(R.n_regions, _p(R.start), _p(R.type), _p(R.info), R.n_anchor_kmers, _p(R.anchor_kmers), R.k, _p(R.contig4))
    A = reads_struct(c.reads)
    valid, s = np.full(R.n_regions, 9, dtype=np.uint8), ArmsSummary()
    f = lib.hypo_gpu_arms_build_long if c.long_mode else lib.hypo_gpu_arms_build
    assert f(C.byref(RS), None if resident else C.byref(A), _p(valid), C.byref(s)) == abi.HYPO_OK, lib.hypo_gpu_last_error()
    return valid, dict(n_windows=s.n_windows, n_arms=s.n_arms, arms2_bytes=s.arms2_bytes, draft4_bytes=s.draft4_bytes, out_bytes=s.out_bytes)


def download(lib, summary, long_mode):
    out = dict(windows=np.full(summary["n_windows"], 0xEE, dtype=np.uint8).repeat(40).view(cases.WINDOW_DTYPE), win_region=np.full(summary["n_windows"], 0xDEAD, dtype=np.uint32),
               arm_len=np.full(summary["n_arms"], 0xDEAD, dtype=np.uint32), arm_off=np.full(summary["n_arms"], 0xDEAD, dtype=np.uint64),
               arms2=np.full(summary["arms2_bytes"], 0xEE, dtype=np.uint8), draft4=np.full(summary["draft4_bytes"], 0xEE, dtype=np.uint8))
    f = lib.hypo_gpu_arms_download_long if long_mode else lib.hypo_gpu_arms_download
    assert f(*[_p(out[k]) for k in FIELDS]) == abi.HYPO_OK, lib.hypo_gpu_last_error()
    return out


def assert_equals_the_checker(c, x, valid, summary, got):
    """byte for byte; a difference is reported with the region and type of the window, and for an arm the alignment it is from"""
    R = c.regions
    want = cases.as_arrays(x)
    where = lambda w: f"region {w} ({cases.ac.TYPE_NAMES[int(R.type[w])]}, [{int(R.start[w])}, {int(R.start[w + 1])}))"
    bad = np.nonzero(valid != np.array(x.region_valid, dtype=np.uint8))[0]
    if bad.size:
        w = int(bad[0])
        raise AssertionError(f"region_valid differs in {bad.size} regions, the first {where(w)}: the device has {int(valid[w])}; the checker's counts {x.trace['windows'].get(w)}")
    assert summary == x.summary, f"summary: the device has {summary}, the checker {x.summary}"
    for f in ("win_region", "windows"):
        bad = np.nonzero(got[f] != want[f])[0]
        if bad.size:
            i = int(bad[0])
            raise AssertionError(f"{f}: {bad.size} of {want[f].size} entries differ, the first is window {i}, {where(x.win_region[i])}: the device has {got[f][i]}, the checker {want[f][i]}")
    owner = np.zeros(len(x.arm_len), dtype=np.int64)                              # arm -> window
    origin = []
    for i, v in enumerate(x.windows):
        owner[v["first_arm"]:v["first_arm"] + v["n_internal"] + v["n_prefix"] + v["n_suffix"]] = i
        origin += x.trace["windows"][v["region"]]["kept_from"]
    for f in ("arm_len", "arm_off"):
        bad = np.nonzero(got[f] != want[f])[0]
        if bad.size:
            i = int(bad[0])
            raise AssertionError(f"{f}: {bad.size} of {want[f].size} entries differ, the first is arm {i} ({origin[i][0]}, from alignment {origin[i][1]}) of {where(x.win_region[owner[i]])}: "
                                 f"the device has {int(got[f][i])}, the checker {int(want[f][i])}")
    bad = np.nonzero(got["arms2"] != want["arms2"])[0]
    if bad.size:
        i = int(np.searchsorted(want["arm_off"], bad[0], "right")) - 1
        raise AssertionError(f"arms2: {bad.size} of {want['arms2'].size} bytes differ, the first is byte {int(bad[0]) - int(want['arm_off'][i])} of arm {i} ({origin[i][0]}, from alignment "
                             f"{origin[i][1]}) of {where(x.win_region[owner[i]])}: the device has {int(got['arms2'][bad[0]]):#04x}, the checker {int(want['arms2'][bad[0]]):#04x}")
    bad = np.nonzero(got["draft4"] != want["draft4"])[0]
    if bad.size:
        i = int(np.searchsorted(want["windows"]["draft_off"], bad[0], "right")) - 1
        raise AssertionError(f"draft4: {bad.size} of {want['draft4'].size} bytes differ, the first in window {i}, {where(x.win_region[i])}")


def run(lib, name, resident=False):
    c, x = cases.case(name), cases.expected(name)
    valid, summary = build(lib, c, resident)
    got = download(lib, summary, c.long_mode)
    assert_equals_the_checker(c, x, valid, summary, got)
    return c, x, summary, got


def host_batch(summary, got):
    s = abi.WindowBatch()
    s.n_windows, s.n_arms = summary["n_windows"], summary["n_arms"]
    s.windows, s.draft4, s.draft4_bytes = _p(got["windows"]), _p(got["draft4"]), got["draft4"].size
    s.arm_off, s.arm_len, s.arms2, s.arms2_bytes = _p(got["arm_off"]), _p(got["arm_len"]), _p(got["arms2"]), got["arms2"].size
    return s


@pytest.mark.parametrize("name", cases.CASES)
def test_the_batch_equals_the_checker(lib, name):
    """corners: break points decided in every way; empty_arms: windows deleted whole; anchors_k*: every outcome of the four searches of
    prepare_short_arm; pruning / long_pruning: a window either side of every threshold; file_order / long_file_order: arms placed by
    file_rank; span_search: the alignments a window looks at; packing: every offset of a window and of an arm; two_contigs; blocks /
    many_regions: prefix sums over more than one block and more than 1024 blocks; long_*: the cuts of find_long_arms and the filter"""
    cases.condition(name)
    c, x, summary, got = run(lib, name)
    # the consensus slots are laid out by hypo_gpu_poa_slot_layout's rule
    off = np.zeros(summary["n_windows"] + 1, dtype=np.uint64)
    b = host_batch(summary, got)
    assert lib.hypo_gpu_poa_slot_layout(C.byref(b), _p(off)) == abi.HYPO_OK
    assert int(off[-1]) == summary["out_bytes"]


@pytest.mark.parametrize("name", ["corners", "anchors_k13"])
def test_resident_reads_give_the_same_batch(lib, name):
    """hypo_gpu_reads_upload, then hypo_gpu_arms_build(regions, NULL, ...): the same download as with the reads handed over"""
    c = cases.case(name)
    _, _, summary, got = run(lib, name)
    A = reads_struct(c.reads)
    ctg = np.zeros(c.reads.rb.size, dtype=np.uint32)
    assert lib.hypo_gpu_reads_upload(C.byref(A), _p(ctg), C.c_uint64(int(c.regions.start[-1]))) == abi.HYPO_OK, lib.hypo_gpu_last_error()
    _, _, summary2, got2 = run(lib, name, resident=True)
    assert summary2 == summary and all((got2[f] == got[f]).all() for f in FIELDS)


def test_short_and_long_batches_live_side_by_side(lib):
    """a short build, a long build, a second short build of another case: every download is its own checker's, and the long batch is
    what it was after the second short build"""
    run(lib, "packing")
    c, x, summary, got = run(lib, "long_geometry")
    run(lib, "empty_arms")
    again = download(lib, summary, True)
    assert all((again[f] == got[f]).all() for f in FIELDS)
    assert_equals_the_checker(c, x, np.array(x.region_valid, dtype=np.uint8), summary, again)
    short = download(lib, cases.expected("empty_arms").summary, False)
    assert_equals_the_checker(cases.case("empty_arms"), cases.expected("empty_arms"), np.array(cases.expected("empty_arms").region_valid, dtype=np.uint8),
                              cases.expected("empty_arms").summary, short)


def test_the_resident_batch_polishes_like_its_downloaded_copy(lib):
    """hypo_gpu_arms_poa on the resident batch of `pruning` against hypo_gpu_poa_batch on what hypo_gpu_arms_download gave: the same
    bases, lengths and statuses"""
    _, x, summary, got = run(lib, "pruning")
    n = summary["n_windows"]
    assert n >= 25 and summary["n_arms"] > 200
    sp = abi.ScoreParams(*abi.DEFAULT_SCORES)
    bases = np.zeros(summary["out_bytes"] + 1, dtype=np.uint8); off = np.zeros(n + 1, dtype=np.uint64)
    ln = np.full(n, 0xDEAD, dtype=np.uint32); st = np.full(n, 0xEE, dtype=np.uint8)
    assert lib.hypo_gpu_arms_poa(C.byref(sp), _p(bases), _p(off), _p(ln), _p(st)) == abi.HYPO_OK, lib.hypo_gpu_last_error()
    b = host_batch(summary, got)
    off2 = np.zeros(n + 1, dtype=np.uint64)
    assert lib.hypo_gpu_poa_slot_layout(C.byref(b), _p(off2)) == abi.HYPO_OK
    assert (off == off2).all()
    bases2 = np.zeros(int(off2[-1]) + 1, dtype=np.uint8); ln2 = np.full(n, 0xDEAD, dtype=np.uint32); st2 = np.full(n, 0xEE, dtype=np.uint8)
    out = abi.ConsensusBatch(_p(bases2), _p(off2), _p(ln2), _p(st2))
    assert lib.hypo_gpu_poa_batch(C.byref(sp), C.byref(b), C.byref(out)) == abi.HYPO_OK, lib.hypo_gpu_last_error()
    assert (st == st2).all() and (ln == ln2).all() and (st == 0).all() and (ln > 0).all()
    for i in range(n):
        assert (bases[int(off[i]):int(off[i]) + int(ln[i])] == bases2[int(off2[i]):int(off2[i]) + int(ln2[i])]).all(), f"window {i}"
