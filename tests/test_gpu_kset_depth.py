"""GPU: hypo_gpu_kset_query_depth (kset_kernel.hip, hypo --qv-cn) against the CPU checker (tests/cn_checker.py), as exact
integers.  One set per k: a 12 kbp genome read 8 times, one stretch 16 times (a collapsed repeat when the text has it once), one
once and one 3 times (the least counts 2 and 5), a k-mer read 300 times; plane 0 holds the genome with one stretch twice (a
duplication) and a k-mer 300 times, plane 1 another text.  The queries are the smallest shapes that cross every path of the kernel:
bins below, at and above the 2048 window starts of a wave's pass, sequences of 0, k - 1, k, bin - 1, bin, bin + 1, bin + k - 1 and
2 bin bytes and of a few thousand, empty ones between them, a bin without a window, non-ACGT bytes and lower case."""
import ctypes as C

import numpy as np
import pytest

import cn_checker as cn
import test_gpu_kset as tk
from hypo_amd import abi

pytestmark = pytest.mark.gpu
KS = [12, 21, 31]
BINS = [32, 100, 1024]
MORE_BINS = [2048, 5000]            # at and above a pass (k = 21 only)
UNIT = 8
COLS = ("windows", "missing", "rated", "over", "under", "med_count")
# the genome's stretches and how often the reads hold them
DEPTHS = [(0, 1000, 8), (1000, 1800, 16), (1800, 3000, 8), (3000, 3300, 1), (3300, 3600, 3), (3600, 12000, 8)]
COLLAPSED, DUPLICATED = (1000, 1800), (4000, 4700)


@pytest.fixture(scope="module")
def gpu():
    from hypo_amd import capi
    g = capi.HypoGpu(0)
    yield g
    if LIVE[0] is not None:
        LIVE[0] = None
        g.kset_end()


class Case:
    def __init__(self, k):
        rng = np.random.default_rng(7100 + k)
        self.k = k
        self.g = g = tk.rnd(rng, 12000)
        self.x, self.y = tk.rnd(rng, k), tk.rnd(rng, k)                 # read 300 times; 300 times in the text
        recs = []
        for a, b, d in DEPTHS:
            recs += [g[a:b + k - 1]] * d                                # (the windows over a seam go with the stretch on their left)
        recs += [self.x] * 300 + [self.y] * 8 + [tk.mutate(rng, g[5000:5600], 0.02)]
        self.recs = recs
        self.reads = cn.tally(recs, k)
        self.marks = ([g, g[DUPLICATED[0]:DUPLICATED[1]], self.x] + [self.y] * 300, [g[:3000], g[2000:2500].lower()])
        self.texts = [cn.tally(m, k) for m in self.marks]
        assert self.reads[cn.windows(self.x, k)[0][1]] == 255 and self.texts[0][cn.windows(self.y, k)[0][1]] == 255


CASES = {}
LIVE = [None]                       # the k whose set is on the device


def ready(gpu, k):
    """the case of k with its set on the device, both planes marked and the least count at 1"""
    c = CASES.setdefault(k, Case(k))
    if LIVE[0] != k:
        LIVE[0] = None
        gpu.kset_begin(k, len(c.reads))
        gpu.kset_counts_enable(2)
        gpu.kset_add(b"\n".join(c.recs))
        assert gpu.kset_size()[0] == len(c.reads)
        for t, m in enumerate(c.marks):
            gpu.kset_mark(t, m)
        LIVE[0] = k
    gpu.kset_min_count(1)
    return c


def queries(c, bin):
    g, k = c.g, c.k
    odd = bytearray(g[6000:6400])
    odd[50], odd[51], odd[200] = ord("N"), ord("n"), ord("R")
    return [b"", g[:k - 1], b"", g[10:10 + k], g[20:20 + bin - 1], g[100:100 + bin], b"", g[300:300 + bin + 1], g[1000:1000 + bin + k - 1],
            g[2000:2000 + 2 * bin], bytes(odd), g[700:1300].lower(), c.x + b"N" + c.y, c.x, b"N" * 40, b"", g[500:5000], b""]


def check(gpu, c, seqs, bin, text, unit, t=1):
    got = gpu.kset_query_depth(seqs, bin=bin, text=text, unit=unit)
    want = cn.depth(seqs, c.k, bin, c.reads, c.texts[text], unit, t)
    assert got[0].size == len(want["windows"]) == sum(cn.n_bins(len(s), bin) for s in seqs)
    for name, a in zip(COLS, got):
        bad = np.flatnonzero(a.astype(np.int64) != np.array(want[name], np.int64))
        assert bad.size == 0, (name, bin, text, unit, t, bad[:8], a[bad[:8]], [want[name][i] for i in bad[:8]])
    return want


@pytest.mark.parametrize("bin", BINS)
@pytest.mark.parametrize("k", KS)
def test_against_the_checker(gpu, k, bin):
    c = ready(gpu, k)
    seqs = queries(c, bin)
    want = check(gpu, c, seqs, bin, 0, UNIT)
    assert sum(want["over"]) > 0 and sum(want["under"]) > 0 and 255 in want["med_count"] and 0 in want["windows"]
    # per sequence the missing windows are those of hypo_gpu_kset_query
    total, missing = gpu.kset_query(seqs)
    first = np.cumsum([0] + [cn.n_bins(len(s), bin) for s in seqs])
    assert [sum(want["missing"][a:b]) for a, b in zip(first, first[1:])] == missing.tolist()
    assert [sum(want["windows"][a:b]) for a, b in zip(first, first[1:])] == total.tolist()
    check(gpu, c, seqs, bin, 1, UNIT)                                   # the other plane, marked with another text
    check(gpu, c, seqs, bin, 0, 3)
    check(gpu, c, seqs, bin, 1, 255)


@pytest.mark.parametrize("bin", MORE_BINS)
def test_bins_at_and_above_a_pass(gpu, bin):
    c = ready(gpu, 21)
    check(gpu, c, queries(c, bin) + [c.g], bin, 0, UNIT)


@pytest.mark.parametrize("k", KS)
def test_min_count(gpu, k):
    c = ready(gpu, k)
    seqs = [c.g[2800:3800], c.g[:400]]
    try:
        seen = []
        for t in (1, 2, 5):
            gpu.kset_min_count(t)
            seen.append(sum(check(gpu, c, seqs, 100, 0, UNIT, t)["missing"]))
        assert seen[0] == 0 and seen[1] >= 300 - k and seen[2] >= seen[1] + 300 - k     # the stretches read once and 3 times go
    finally:
        gpu.kset_min_count(1)


@pytest.mark.parametrize("k", KS)
def test_collapsed_duplicated_and_a_bin_of_both(gpu, k):
    c = ready(gpu, k)
    g, bin = c.g, 100
    col, dup = g[COLLAPSED[0]:COLLAPSED[1]], g[DUPLICATED[0]:DUPLICATED[1]]
    # a bin of both: p - k + 1 windows of the stretch read twice as deep, as many of the stretch the text has twice, and between
    # them the windows over the seam, which no read has (k odd) or which an N takes away (k even)
    p = (99 + k) // 2 if k % 2 else (98 + k) // 2
    half = g[1200:1200 + p] + (b"" if k % 2 else b"N") + g[4100:4100 + (p - k + 1) + k - 1]
    w = check(gpu, c, [col, dup, half], bin, 0, UNIT)
    rows = list(zip(*(w[n] for n in COLS)))
    calls = [cn.call(r[2], r[3], r[4]) for r in rows]
    n_col, n_dup = cn.n_bins(len(col), bin), cn.n_bins(len(dup), bin)
    assert all(r[0] > 0 and r[2] == r[3] == r[0] and r[4] == 0 for r in rows[:n_col]) and calls[:n_col] == ["collapsed"] * n_col
    assert all(r[0] > 0 and r[2] == r[4] == r[0] and r[3] == 0 for r in rows[n_col:n_col + n_dup]) and calls[n_col:n_col + n_dup] == ["duplicated"] * n_dup
    both = rows[n_col + n_dup]
    assert both[3] == both[4] == p - k + 1 and both[2] == 2 * both[3] and calls[n_col + n_dup] == "."
    assert [r[5] for r in rows[:n_col]] == [16] * n_col and [r[5] for r in rows[n_col:n_col + n_dup]] == [8] * n_dup


@pytest.mark.parametrize("bin", BINS)
def test_a_long_sequence_in_pieces(gpu, bin):
    """cut at multiples of bin with k - 1 bytes of overlap, the pieces' arrays concatenate to the single call's (the bin the
    overlap alone opens holds no window and is dropped)"""
    c = ready(gpu, 21)
    k, long = c.k, c.g[500:5000]
    whole = gpu.kset_query_depth([long], bin=bin, text=0, unit=UNIT)
    step = 7 * bin if bin < 1024 else 2 * bin
    parts = [[] for _ in COLS]
    for lo in range(0, len(long), step):
        last = lo + step >= len(long)
        got = gpu.kset_query_depth([long[lo:len(long) if last else lo + step + k - 1]], bin=bin, text=0, unit=UNIT)
        keep = got[0].size if last else step // bin
        if not last:
            assert got[0].size == keep + 1 and not any(a[keep] for a in got)
        for p, a in zip(parts, got):
            p.append(a[:keep])
    for name, p, a in zip(COLS, parts, whole):
        assert np.array_equal(np.concatenate(p), a), (name, bin)


def test_same_answer_twice_and_the_set_untouched(gpu):
    c = ready(gpu, 21)
    seqs = queries(c, 100)
    before = (gpu.kset_spectrum(0), gpu.kset_spectrum(1), gpu.kset_export()[:3], gpu.kset_size())
    a = gpu.kset_query_depth(seqs, bin=100, text=0, unit=UNIT)
    b = gpu.kset_query_depth(seqs, bin=100, text=0, unit=UNIT)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    after = (gpu.kset_spectrum(0), gpu.kset_spectrum(1), gpu.kset_export()[:3], gpu.kset_size())
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and before[3] == after[3]
    assert np.array_equal(before[2][0], after[2][0]) and np.array_equal(before[2][1], after[2][1]) and before[2][2] == after[2][2]


def untouched(out):
    return all((a == abi.DEPTH_UNTOUCHED32).all() for a in out[1:6]) and (out[6] == abi.DEPTH_UNTOUCHED8).all()


def test_refused_calls_change_nothing(gpu):
    c = ready(gpu, 21)
    text = c.g[:300]
    off = np.array([0, 100, 300], np.uint64)
    ok = gpu.kset_query_depth_rc(text, off, bin=32, text=0, unit=UNIT)
    assert ok[0] == abi.HYPO_OK and ok[1].size == 4 + 7 and not untouched(ok)
    refused = [dict(bin=31), dict(bin=65537), dict(bin=0), dict(unit=0), dict(unit=256), dict(text=2), dict(text=4), dict(n_bins=10), dict(n_bins=12),
               dict(n_bins=0)]
    for kw in refused:
        args = dict(bin=32, text=0, unit=UNIT)
        args.update(kw)
        out = gpu.kset_query_depth_rc(text, off, **args)
        assert out[0] == abi.HYPO_E_INVALID and untouched(out), kw
    out = gpu.kset_query_depth_rc(text, np.array([0, 200, 100], np.uint64), bin=32, text=0, unit=UNIT, n_bins=11)
    assert out[0] == abi.HYPO_E_INVALID and untouched(out) and b"decrease" in gpu.lib.hypo_gpu_last_error()
    # a NULL required pointer with n_bins > 0
    buf = np.frombuffer(text, np.uint8)
    arrays = [np.full(11, abi.DEPTH_UNTOUCHED32, np.uint32) for _ in range(5)] + [np.full(11, abi.DEPTH_UNTOUCHED8, np.uint8)]
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for null in range(6):
        ptrs = [None if i == null else p(a) for i, a in enumerate(arrays)]
        rc = gpu.lib.hypo_gpu_kset_query_depth(p(buf), p(off), C.c_uint32(2), C.c_uint32(32), C.c_uint32(0), C.c_uint32(UNIT), C.c_uint64(11), *ptrs)
        assert rc == abi.HYPO_E_INVALID and untouched([rc] + arrays), null
    for ptrs in ([None, p(off)], [p(buf), None]):
        rc = gpu.lib.hypo_gpu_kset_query_depth(*ptrs, C.c_uint32(2), C.c_uint32(32), C.c_uint32(0), C.c_uint32(UNIT), C.c_uint64(11), *[p(a) for a in arrays])
        assert rc == abi.HYPO_E_INVALID and untouched([rc] + arrays)
    # n_seqs == 0 touches nothing
    rc = gpu.lib.hypo_gpu_kset_query_depth(None, None, C.c_uint32(0), C.c_uint32(32), C.c_uint32(0), C.c_uint32(UNIT), C.c_uint64(0), *[p(a) for a in arrays])
    assert rc == abi.HYPO_OK and untouched([rc] + arrays)
    # empty sequences only: no bin, nothing written
    out = gpu.kset_query_depth_rc([b"", b""], bin=32, text=0, unit=UNIT)
    assert out[0] == abi.HYPO_OK and out[1].size == 0


def test_needs_a_set_that_counts(gpu):
    LIVE[0] = None
    text, off = b"ACGT" * 30, np.array([0, 120], np.uint64)
    gpu.kset_begin(21, 100)
    try:
        gpu.kset_add(text)
        out = gpu.kset_query_depth_rc(text, off, bin=32, text=0, unit=UNIT)
        assert out[0] == abi.HYPO_E_INVALID and untouched(out) and b"counts" in gpu.lib.hypo_gpu_last_error()
    finally:
        gpu.kset_end()
    out = gpu.kset_query_depth_rc(text, off, bin=32, text=0, unit=UNIT)
    assert out[0] == abi.HYPO_E_INVALID and untouched(out) and b"no k-mer set" in gpu.lib.hypo_gpu_last_error()
