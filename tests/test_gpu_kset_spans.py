"""GPU: hypo_gpu_kset_query_spans (kset_kernel.hip, the spans kernel) against qv_checker.seq_stats of every span's bytes, as exact
integers, for both lane-group widths the library can launch (a half-wave per span is the default, HYPO_KSET_SPAN_GROUP=64 gives a
wave per span).  R: the reads of tests/test_gpu_kset.py (20 kbp at 30x, with that file's oddities)."""
import ctypes as C
import os

import numpy as np
import pytest

import qv_checker as qc
from test_gpu_kset import mutate, palindrome, read_records, rnd

pytestmark = pytest.mark.gpu
KS = [12, 21, 22, 31]
GROUPS = [32, 64]


@pytest.fixture(scope="module")
def gpu():
    from hypo_amd import capi
    return capi.HypoGpu(0)


@pytest.fixture(scope="module")
def piece():
    from hypo_amd import capi
    return capi.KSET_SPAN_PIECE


@pytest.fixture
def group(request):
    old = os.environ.get("HYPO_KSET_SPAN_GROUP")
    os.environ["HYPO_KSET_SPAN_GROUP"] = str(request.param)
    yield request.param
    if old is None:
        del os.environ["HYPO_KSET_SPAN_GROUP"]
    else:
        os.environ["HYPO_KSET_SPAN_GROUP"] = old


_cases = {}


def case(k, piece):
    """(read blob, R, text, [(name, lo[], hi[])], {name: (total[], missing[])}) of one k, built once"""
    if k in _cases:
        return _cases[k]
    rng = np.random.default_rng(4000 + k)
    genome, recs = read_records(rng, k)
    R = qc.read_set(recs, k)
    t = bytearray(mutate(rng, genome, 0.01) + rnd(rng, 3000) + mutate(rng, genome[:3000], 0.03))
    t[1000:1001] = b"N"; t[1060:1061] = b"N"                       # a span that starts and ends with N
    t[1100:1101] = bytes(t[1100:1101]).lower(); t[1160:1161] = bytes(t[1160:1161]).lower()
    t[1300:1400] = b"N" * 100
    t[1500:1600] = bytes(t[1500:1600]).lower()
    t[1700:1703] = b"RYK"
    pal = palindrome(k - k % 2)
    t[2000:2000 + len(pal)] = pal
    text = bytes(t)
    n = len(text)
    W = lambda w: w + k - 1                                          # the length of a span with w windows
    edge = [(5, 5), (7, 7 + k - 1), (9, 9 + k), (11, 11 + k + 1), (0, 0), (n, n), (0, k), (n - k, n), (0, 300), (n - 300, n), (0, n)]
    counts = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, piece - 1, piece, piece + 1, 2 * piece - 1, 2 * piece, 2 * piece + 1]
    edge += [(a, a + W(w)) for w in counts for a in (0, 3000 + w, n - W(w))]
    edge += [(1000, 1061), (1000, 1000 + k), (1061 - k, 1061), (1100, 1161), (1100, 1100 + k), (1161 - k, 1161), (1300, 1400), (1310, 1350),
             (1290, 1410), (1500, 1600), (1490, 1610), (1690, 1720), (2000, 2000 + len(pal)), (1990, 2010 + len(pal))]
    edge += [(4000, 4090)] * 3                                                            # identical
    edge += [(5000, 5200), (5010, 5190), (5050, 5050 + k), (5000, 5100), (5100, 5200)]   # nested
    tile = 40 + k
    edge += [(6000 + i * (tile - k + 1), 6000 + i * (tile - k + 1) + tile) for i in range(40)]   # neighbours share k - 1 bytes
    order = rng.permutation(len(edge))
    short_lo = rng.integers(0, n - 60, 5000)
    short = list(zip(short_lo.tolist(), (short_lo + rng.integers(40, 61, 5000)).tolist()))
    one_long = short[:2500] + [(100, 20100)] + short[2500:]
    sets = [("edge", edge), ("edge shuffled", [edge[i] for i in order]), ("one long among short", one_long)]
    sets = [(name, np.array([a for a, _ in s], np.uint64), np.array([b for _, b in s], np.uint64)) for name, s in sets]
    memo = {}

    def ref(a, b):
        if (a, b) not in memo:
            memo[(a, b)] = qc.seq_stats(text[a:b], k, R)
        return memo[(a, b)]
    want = {name: tuple(np.array(x, np.uint64) for x in zip(*[ref(int(a), int(b)) for a, b in zip(lo, hi)])) for name, lo, hi in sets}
    for tot, mis in want.values():
        tot.setflags(write=False); mis.setflags(write=False)
    assert want["edge"][0][:4].tolist() == [0, 0, 1, 2] and 0 < want["edge"][1].sum() < want["edge"][0].sum()
    _cases[k] = (b"\n".join(recs), R, text, sets, want)
    return _cases[k]


@pytest.mark.parametrize("group", GROUPS, indirect=True)
@pytest.mark.parametrize("k", KS)
def test_spans_equal_checker(gpu, piece, k, group):
    blob, R, text, sets, want = case(k, piece)
    gpu.kset_begin(k, R.size)
    try:
        gpu.kset_add(blob)
        assert gpu.kset_size()[0] == R.size
        for name, lo, hi in sets:
            total, missing = gpu.kset_query_spans(text, lo, hi)
            bad = np.flatnonzero((total != want[name][0]) | (missing != want[name][1]))
            assert bad.size == 0, (name, [(int(lo[i]), int(hi[i]), int(total[i]), int(missing[i]), int(want[name][0][i]), int(want[name][1][i])) for i in bad[:5]])
            again = gpu.kset_query_spans(text, lo, hi)                                   # the same spans give the same arrays
            assert np.array_equal(again[0], total) and np.array_equal(again[1], missing)
        # n_spans of 0, 1 and one more than a workgroup's share (256 lanes / the group width)
        name, lo, hi = sets[1]
        for n in (0, 1, 256 // group, 256 // group + 1):
            total, missing = gpu.kset_query_spans(text, lo[:n], hi[:n])
            assert total.tolist() == want[name][0][:n].tolist() and missing.tolist() == want[name][1][:n].tolist()
        # the span query and the sequence query agree
        some = [(int(a), int(b)) for a, b in zip(lo[:50], hi[:50])]
        tq, mq = gpu.kset_query([text[a:b] for a, b in some])
        ts, ms = gpu.kset_query_spans(text, lo[:50], hi[:50])
        assert tq.tolist() == ts.tolist() and mq.tolist() == ms.tolist()
        # a text shorter than k, and an empty one
        assert [x.tolist() for x in gpu.kset_query_spans(b"ACGT", [0, 1], [4, 3])] == [[0, 0], [0, 0]]
        assert [x.tolist() for x in gpu.kset_query_spans(b"", [0], [0])] == [[0], [0]]
    finally:
        gpu.kset_end()


def test_palindrome_at_even_k(gpu):
    for k in (12, 22):
        pal = palindrome(k)
        gpu.kset_begin(k, 10)
        try:
            gpu.kset_add(b"GG" + pal + b"TT")
            text = b"N" + pal.lower() + b"A" + pal
            total, missing = gpu.kset_query_spans(text, [1, k + 2, 0, 1], [k + 1, 2 * k + 2, len(text), k + 2])
            R = qc.read_set([b"GG" + pal + b"TT"], k)
            want = [qc.seq_stats(text[a:b], k, R) for a, b in ((1, k + 1), (k + 2, 2 * k + 2), (0, len(text)), (1, k + 2))]
            assert list(zip(total.tolist(), missing.tolist())) == want and want[0] == (1, 0) and want[1] == (1, 0)
        finally:
            gpu.kset_end()


def test_argument_errors(gpu):
    from hypo_amd import abi
    lib = gpu.lib
    text = b"ACGTTGCA" * 8
    rc, _, _ = gpu.kset_query_spans_rc(text, [0], [40])
    assert rc == abi.HYPO_E_INVALID and b"hypo_gpu_kset_begin" in lib.hypo_gpu_last_error()          # no set, as hypo_gpu_kset_query
    gpu.kset_begin(12, 100)
    try:
        gpu.kset_add(text)
        ok = gpu.kset_query_spans(text, [0, 8], [64, 40])
        for lo, hi in (([0, 41], [64, 40]), ([0, 8], [65, 40]), ([0, 65], [64, 65]), ([2 ** 63], [2 ** 63 + 20]), ([30], [2 ** 64 - 1])):
            rc, _, _ = gpu.kset_query_spans_rc(text, lo, hi)
            assert rc == abi.HYPO_E_INVALID, (lo, hi)
        assert gpu.kset_query_spans_rc(text, [64], [64])[0] == 0                                          # empty at the end is a span
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        lo, hi, out = np.zeros(1, np.uint64), np.full(1, 40, np.uint64), np.zeros(2, np.uint64)
        call = lambda b, l, h, t, m, n=1: lib.hypo_gpu_kset_query_spans(b, C.c_uint64(64), l, h, C.c_uint32(n), t, m)
        assert call(text, None, p(hi), p(out), p(out[1:])) == abi.HYPO_E_INVALID
        assert call(text, p(lo), None, p(out), p(out[1:])) == abi.HYPO_E_INVALID
        assert call(text, p(lo), p(hi), None, p(out[1:])) == abi.HYPO_E_INVALID
        assert call(text, p(lo), p(hi), p(out), None) == abi.HYPO_E_INVALID
        assert call(None, p(lo), p(hi), p(out), p(out[1:])) == abi.HYPO_E_INVALID
        assert call(None, None, None, None, None, n=0) == 0                                               # no span: nothing to do
        after = gpu.kset_query_spans(text, [0, 8], [64, 40])                                              # refused calls change nothing
        assert [x.tolist() for x in after] == [x.tolist() for x in ok] == [[53, 21], [0, 0]]
    finally:
        gpu.kset_end()
