"""GPU: the host paths of the k-mer set's entry points that rebase what the caller hands in, which no other test reaches: offsets
that do not start at 0 (`bytes + off[0]` and the relative offsets of hypo_gpu_kset_query, _query_track and _mark) and an edit_off[]
that does not start at 0 (hypo_gpu_kset_query_variants reads eb / ee / ao / al from edit_off[0] on).  Every answer of the shifted
call equals that of the zero-based call, as exact integers.  The shapes are the smallest that reach those paths: 600 bytes in four
sequences (one empty, one shorter than k, one with an N), two sites of one and two edits."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
KS = [12, 31]
JUNK = b"GATTACA"                                                       # 7 bytes in front of the text: bases, so a call that read them would count them
CUTS = [0, 250, 250, 259, 600]                                          # four sequences: 250 bytes (the N is in it), none, 9 < k, 341
E_FIRST = 3                                                             # entries of eb / ee / ao / al in front of the first site's edits


@pytest.fixture(scope="module")
def gpu():
    from hypo_amd import capi
    return capi.HypoGpu(0)


@functools.lru_cache(maxsize=None)
def case(k):
    """(text, reads): 600 random bases with one N; the reads are the text with a handful of substitutions"""
    rng = np.random.default_rng(4100 + k)
    text = bytearray(rng.choice(list(b"ACGT"), CUTS[-1]).astype(np.uint8).tobytes())
    text[100] = ord("N")
    reads = bytearray(text)
    for p in (40, 180, 255, 300, 420, 590):
        reads[p] = b"ACGT"[(b"ACGT".index(reads[p]) + 1) % 4]
    return bytes(text), bytes(reads)


def seqs_of(text):
    return [text[a:b] for a, b in zip(CUTS, CUTS[1:])]


def variant_arrays(k):
    """two sites of one and two edits behind E_FIRST entries that no check would let through: (lo, hi, edit_off, eb, ee, ao, al, alts)"""
    alts = b"#T#GG#"
    lo, hi = np.array([300, 400], np.uint64), np.array([300 + 2 * k + 5, 400 + 3 * k], np.uint64)
    edit_off = np.array([E_FIRST, E_FIRST + 1, E_FIRST + 3], np.uint32)
    eb = np.array([9, 9, 9, 300 + k, 400 + 5, 400 + k + 7], np.uint64)
    ee = np.array([1, 1, 1, 300 + k + 1, 400 + 5, 400 + k + 9], np.uint64)      # a substitution, an insertion, a deletion of two
    ao = np.array([1000, 1000, 1000, 1, 3, 5], np.uint64)
    al = np.array([1, 1, 1, 1, 2, 0], np.uint32)
    return lo, hi, edit_off, eb, ee, ao, al, alts


def test_junk_entries_are_invalid_and_variants_have_windows(gpu):
    """the comparison of test_variants_from_edit_off cannot pass vacuously"""
    from hypo_amd import abi
    for k in KS:
        text, reads = case(k)
        lo, hi, edit_off, eb, ee, ao, al, alts = variant_arrays(k)
        assert (eb[:E_FIRST] > ee[:E_FIRST]).all() and (ao[:E_FIRST] > len(alts)).all()
        gpu.kset_begin(k, len(reads))
        try:
            gpu.kset_add(reads)
            for j in range(E_FIRST):                                    # a site that owns junk entry j is refused
                rc = gpu.kset_query_variants_rc(text, alts, lo[:1], hi[:1], np.array([j, j + 1], np.uint32), eb, ee, ao, al)[0]
                assert rc == abi.HYPO_E_INVALID, j
            _, _, _, vt, vm = gpu.kset_query_variants(text, alts, lo, hi, edit_off - E_FIRST, eb[E_FIRST:], ee[E_FIRST:], ao[E_FIRST:], al[E_FIRST:])
            assert vt.size == 2 + 4 and (vt > 0).all() and len(set(vt.tolist())) > 1 and vm.any()
        finally:
            gpu.kset_end()


@pytest.mark.parametrize("k", KS)
def test_query_and_track_from_shifted_offsets(gpu, k):
    text, reads = case(k)
    off = np.array(CUTS, np.uint64)
    shifted = np.frombuffer(JUNK + text + b"\0", np.uint8)
    off7 = off + np.uint64(len(JUNK))
    gpu.kset_begin(k, len(reads))
    try:
        gpu.kset_add(reads)
        total, missing = gpu.kset_query(seqs_of(text))
        assert total[0] > 0 and total[1] == 0 and total[2] == 0 and missing[0] > 0 and missing[3] > 0
        t7, m7 = np.full(4, 99, np.uint64), np.full(4, 99, np.uint64)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        assert gpu.lib.hypo_gpu_kset_query(p(shifted), p(off7), C.c_uint32(4), p(t7), p(m7)) == 0
        assert t7.tolist() == total.tolist() and m7.tolist() == missing.tolist()
        for want in (None, np.array([1, 1, 0, 1], np.uint8)):
            base = gpu.kset_query_track(text, off, want)
            got = gpu.kset_query_track(JUNK + text, off7, want)
            assert base[0].tolist() == total.tolist() and base[1].tolist() == missing.tolist() and base[3].size > 2
            for what, g, e in zip(("total", "missing", "iv_off", "iv_start", "iv_end", "iv_missing"), got, base):
                assert g.tolist() == e.tolist(), what
    finally:
        gpu.kset_end()


@pytest.mark.parametrize("k", KS)
def test_mark_from_shifted_offsets(gpu, k):
    text, reads = case(k)
    shifted = np.frombuffer(JUNK + text + b"\0", np.uint8)
    off7 = np.array(CUTS, np.uint64) + np.uint64(len(JUNK))
    gpu.kset_begin(k, len(reads))
    try:
        gpu.kset_counts_enable(2)
        gpu.kset_add(reads)
        n_win, n_un = C.c_uint64(0), C.c_uint64(0)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        assert gpu.lib.hypo_gpu_kset_mark(C.c_uint32(0), p(shifted), p(off7), C.c_uint32(4), C.byref(n_win), C.byref(n_un)) == 0
        want = gpu.kset_mark(1, seqs_of(text))
        assert (int(n_win.value), int(n_un.value)) == want and want[0] > want[1] > 0
        s0, s1 = gpu.kset_spectrum(0), gpu.kset_spectrum(1)
        assert s1[:, 1:].sum() > 0 and (s0 == s1).all()
    finally:
        gpu.kset_end()


@pytest.mark.parametrize("k", KS)
def test_variants_from_edit_off(gpu, k):
    text, reads = case(k)
    lo, hi, edit_off, eb, ee, ao, al, alts = variant_arrays(k)
    gpu.kset_begin(k, len(reads))
    try:
        gpu.kset_add(reads)
        for variants in (True, False):
            base = gpu.kset_query_variants(text, alts, lo, hi, edit_off - E_FIRST, eb[E_FIRST:], ee[E_FIRST:], ao[E_FIRST:], al[E_FIRST:], variants=variants)
            got = gpu.kset_query_variants(text, alts, lo, hi, edit_off, eb, ee, ao, al, variants=variants)
            for what, g, e in zip(("best_mask", "best_total", "best_missing", "var_total", "var_missing"), got, base):
                assert (g is None and e is None) if not variants and what.startswith("var") else g.tolist() == e.tolist(), what
    finally:
        gpu.kset_end()
