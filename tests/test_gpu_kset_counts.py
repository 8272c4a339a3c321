"""GPU: read counts, copy numbers and the spectrum on the exact k-mer set (hypo_gpu_kset_counts_enable / _mark / _spectrum,
kset_kernel.hip) against the CPU checker (tests/spectra_checker.py), as exact integers.  The shapes are the smallest at which the
kernels can still go wrong: more than one workgroup of 8192 bytes, growth from the smallest table, sequences that end around a
staging boundary, four slots of one 32-bit word counted at once, and keys far beyond 255."""
import functools
import time

import numpy as np
import pytest

import qv_checker as qc
import spectra_checker as spc
import test_gpu_kset as tk

pytestmark = pytest.mark.gpu
KS = [12, 21, 22, 31]


@pytest.fixture(scope="module")
def gpu():
    from hypo_amd import capi
    return capi.HypoGpu(0)


@functools.lru_cache(maxsize=None)
def case(k):
    """reads of a 20 kbp genome at 30x with 1 % error on both strands and the oddities of test_gpu_kset.read_records; the texts
    (the genome; the genome and 3 of its segments again 1, 2 and 5 times: copy numbers 2, 3 and 6); the checker's answers"""
    rng = np.random.default_rng(2000 + k)
    genome, recs = tk.read_records(rng, k)
    keys, counts = spc.read_counts(recs, k)
    texts = ([genome], [genome] + [genome[1000:1400]] + [genome[5000:5300]] * 2 + [genome[9000:9250]] * 5)
    want = []
    for t in texts:
        cn, asm_only = spc.copy_numbers(t, k, keys)
        want.append((spc.spectrum(counts, cn), sum(len(qc.canonical_windows(s, k)) for s in t), asm_only))
    assert want[1][0][:, 2].sum() > 0 and want[1][0][:, 3].sum() > 0 and want[1][0][:, 4].sum() > 0
    assert spc.histogram(want[0][0])[1] > 1000 and spc.histogram(want[0][0])[20:40].sum() > 1000      # errors, and the peak
    return b"\n".join(recs), keys, texts, want


def mark_and_check(gpu, texts, want):
    for t, (seqs, (S, n_win, asm_only)) in enumerate(zip(texts, want)):
        assert gpu.kset_mark(t, seqs) == (n_win, asm_only)
    for t, (S, _, _) in enumerate(want):
        got = gpu.kset_spectrum(t)
        assert got.shape == (256, 5) and not got[0].any()
        assert (got.astype(np.int64) == S).all(), np.argwhere(got.astype(np.int64) != S)[:10]


@pytest.mark.parametrize("k", KS)
def test_spectrum_and_marks(gpu, k):
    blob, keys, texts, want = case(k)
    gpu.kset_begin(k, keys.size)
    try:
        gpu.kset_counts_enable(2)
        gpu.kset_add(blob)
        n, table_bytes = gpu.kset_size()
        assert n == keys.size and table_bytes >= 2 * (9 + 2) * n          # every resident byte, at a load of at most one half
        _, missing = gpu.kset_query(texts[1])
        assert int(missing.sum()) == want[1][2]                            # n_unmarked is kset_query's missing
        mark_and_check(gpu, texts, want)
    finally:
        gpu.kset_end()


@pytest.mark.parametrize("k", KS)
def test_counts_move_with_their_keys(gpu, k):
    """the same bytes in 4099-byte adds that overlap by exactly k - 1, into the smallest table: it grows, the spectrum is the same"""
    blob, keys, texts, want = case(k)
    gpu.kset_begin(k, 1)
    try:
        gpu.kset_counts_enable(2)
        sizes, chunk, at = [gpu.kset_size()[1]], 4099, 0
        while True:
            gpu.kset_add(blob[at:at + chunk])
            tb = gpu.kset_size()[1]
            if tb != sizes[-1]:
                sizes.append(tb)
            if at + chunk >= len(blob):
                break
            at += chunk - (k - 1)
        assert len(sizes) >= 4 and sizes == sorted(sizes), sizes          # grew at least three times
        assert gpu.kset_size()[0] == keys.size
        mark_and_check(gpu, texts, want)
    finally:
        gpu.kset_end()


@pytest.mark.parametrize("k", KS)
def test_staging_seams(gpu, k):
    """sequences that end 5 bytes before, exactly at and just after a multiple of the 8192 bytes a workgroup stages, and a window
    that starts in the last byte of a lane's 32-byte stretch, as reads (a separator between two) and as a text (back to back)"""
    rng = np.random.default_rng(3000 + k)
    ends = [8192 - 5, 2 * 8192, 3 * 8192 + 1]

    def layout(sep):
        seqs, at = [], 0
        for e in ends:
            seqs.append(tk.rnd(rng, e - at))
            at = e + sep
        lone = tk.rnd(rng, k)                                              # its only window starts at a position = 31 mod 32
        pad = (31 - at) % 32
        seqs.append(b"N" * pad + lone + b"N" * 3)
        seqs.append(tk.rnd(rng, 100))
        return seqs
    reads, text = layout(1), layout(0)
    keys, counts = spc.read_counts(reads, k)
    cn, asm_only = spc.copy_numbers(text, k, keys)
    gpu.kset_begin(k, 1000)
    try:
        gpu.kset_counts_enable(1)
        gpu.kset_add(b"\n".join(reads))
        assert gpu.kset_size()[0] == keys.size
        assert gpu.kset_mark(0, text) == (sum(len(qc.canonical_windows(s, k)) for s in text), asm_only)
        assert (gpu.kset_spectrum(0).astype(np.int64) == spc.spectrum(counts, cn)).all()
        # the reads as the text: every k-mer is there as often as the reads have it
        gpu.kset_end()
        gpu.kset_begin(k, 1000)
        gpu.kset_counts_enable(1)
        gpu.kset_add(b"\n".join(reads))
        assert gpu.kset_mark(0, reads) == (int(counts.sum()), 0)
        assert (gpu.kset_spectrum(0).astype(np.int64) == spc.spectrum(counts, counts)).all()
    finally:
        gpu.kset_end()


@pytest.mark.parametrize("k", KS)
def test_bytes_of_one_word(gpu, k):
    """about 400 keys in a table of 1024 slots, each added 3 to 300 times in shuffled order: the four bytes of a 32-bit word are
    counted at the same time, and a key beyond 255 stops exactly there.  (A call makes room for one new key per byte position it
    holds before it touches the table, so the calls are short enough for 400 keys and a call to fit 512: the table stays as it is.)"""
    rng = np.random.default_rng(4000 + k)
    kmers = [tk.rnd(rng, k) for _ in range(400)]
    times = rng.integers(3, 301, len(kmers))
    times[:8] = [3, 254, 255, 256, 257, 300, 4, 299]
    order = np.repeat(np.arange(len(kmers)), times - 1)
    rng.shuffle(order)
    order = np.concatenate([np.arange(len(kmers)), order])               # every key once, then the rest of their occurrences
    per_call = (110 + k) // (k + 1)                                      # k-mers with an N between them: at most 111 positions
    calls = [b"N".join(kmers[i] for i in order[at:at + per_call]) for at in range(0, order.size, per_call)]
    assert max(len(c) for c in calls) - k + 1 <= 111
    keys, counts = spc.read_counts([b"N".join(kmers * 300)], k)        # which of them are one canonical k-mer: the checker says
    assert 390 <= keys.size <= 400
    total = np.zeros(keys.size, np.int64)
    for km, t in zip(kmers, times):
        total[np.searchsorted(keys, qc.canonical_windows(km, k)[0])] += t
    gpu.kset_begin(k, 1)
    try:
        gpu.kset_counts_enable(2)
        bytes_at_start = gpu.kset_size()[1]
        assert bytes_at_start == 1024 * 8 + 3 * 1024
        for c in calls:
            gpu.kset_add(c)
        assert gpu.kset_size() == (keys.size, bytes_at_start)
        got = gpu.kset_spectrum(1).astype(np.int64)
        assert (got == spc.spectrum(np.minimum(total, 255), np.zeros(keys.size, np.int64))).all()
        assert got[255, 0] == np.count_nonzero(total >= 255) >= 4
    finally:
        gpu.kset_end()


@pytest.mark.parametrize("k", KS)
def test_contention(gpu, k):
    """poly-A, poly-AC and one read 200 000 times: every count is 255, and no lane waits for another"""
    rng = np.random.default_rng(5000 + k)
    hot = tk.rnd(rng, 150)
    parts = [b"A" * 200000, b"AC" * 100000, hot]
    keys, once = spc.read_counts(parts, k)
    assert once.min() >= 1                                                 # (hot's k-mers: 200 000 times what one copy has)
    blob = b"\n".join(parts[:2]) + b"\n" + (hot + b"\n") * (2 * 10 ** 5)
    gpu.kset_begin(k, 1)
    try:
        gpu.kset_counts_enable(1)
        t0 = time.time()
        gpu.kset_add(blob)
        assert time.time() - t0 < 30
        assert gpu.kset_size()[0] == keys.size
        want = np.zeros((256, 5), np.int64)
        want[255, 0] = keys.size
        assert (gpu.kset_spectrum(0).astype(np.int64) == want).all()
        assert gpu.kset_mark(0, [b"A" * 1000]) == (1000 - k + 1, 0)
        want[255, 0] -= 1
        want[255, 4] = 1
        assert (gpu.kset_spectrum(0).astype(np.int64) == want).all()
    finally:
        gpu.kset_end()


@pytest.mark.parametrize("k", KS)
def test_presence_is_what_it_was(gpu, k):
    """with counts on, the three queries answer what they answer on a set of the same reads that does not count"""
    blob, keys, texts, _ = case(k)
    rng = np.random.default_rng(6000 + k)
    genome = texts[0][0]
    qs = [genome, tk.mutate(rng, genome, 0.01), tk.rnd(rng, 3000), b"", tk.rnd(rng, k - 1), b"acgtn" * 30, tk.rnd(rng, 9000, b"ACGTN")]
    text = b"".join(qs)
    lo = rng.integers(0, len(text) - 200, 300)
    hi = lo + rng.integers(0, 200, 300)

    def answers():
        out = [x.tolist() for x in gpu.kset_query(qs)]
        out += [x.tolist() for x in gpu.kset_query_spans(text, lo, hi)]
        out += [x.tolist() for x in gpu.kset_query_track(qs)]
        return out
    gpu.kset_begin(k, keys.size)
    try:
        gpu.kset_add(blob)
        plain = answers()
        gpu.kset_end()
        gpu.kset_begin(k, 1)
        gpu.kset_counts_enable(2)
        gpu.kset_add(blob)
        assert answers() == plain
        gpu.kset_mark(1, qs)
        assert answers() == plain
    finally:
        gpu.kset_end()


def test_argument_errors(gpu):
    from hypo_amd import abi
    lib = gpu.lib
    inv = abi.HYPO_E_INVALID
    assert gpu.kset_counts_enable_rc(2) == inv and b"hypo_gpu_kset_begin" in lib.hypo_gpu_last_error()       # no set
    assert gpu.kset_mark_rc(0, [b"ACGT" * 10])[0] == inv
    assert gpu.kset_spectrum_rc(0)[0] == inv
    k = 12
    reads = b"ACGTTGCAAGGCTTAACCGGATATCGCGTA"
    gpu.kset_begin(k, 10)
    try:
        assert gpu.kset_mark_rc(0, [reads])[0] == inv and b"hypo_gpu_kset_counts_enable" in lib.hypo_gpu_last_error()   # no _enable
        assert gpu.kset_spectrum_rc(0)[0] == inv
        for n in (0, 5):
            assert gpu.kset_counts_enable_rc(n) == inv
        gpu.kset_add(reads)
        assert gpu.kset_counts_enable_rc(2) == inv and b"empty" in lib.hypo_gpu_last_error()                # a set that holds k-mers
        assert gpu.kset_spectrum_rc(0)[0] == inv                           # ... and the refused call enabled nothing
        gpu.kset_add(reads)                                                # ... and closed nothing
    finally:
        gpu.kset_end()
    gpu.kset_begin(k, 10)
    try:
        gpu.kset_counts_enable(2)
        assert gpu.kset_counts_enable_rc(2) == inv                         # twice
        gpu.kset_add(reads)
        keys, counts = spc.read_counts([reads], k)
        zero = np.zeros(keys.size, np.int64)
        assert gpu.kset_spectrum(1).tolist() == spc.spectrum(counts, zero).tolist()
        assert gpu.kset_mark_rc(2, [reads])[0] == inv                      # text = n_texts
        assert gpu.kset_spectrum_rc(2)[0] == inv
        import ctypes as C
        bad = np.array([0, 20, 10], dtype=np.uint64)
        assert lib.hypo_gpu_kset_mark(C.c_uint32(1), reads, bad.ctypes.data_as(C.c_void_p), C.c_uint32(2), None, None) == inv
        gpu.kset_add(reads)                                                # the refused marks did not close the set
        assert gpu.kset_spectrum(1).tolist() == spc.spectrum(2 * counts, zero).tolist()
        assert gpu.kset_mark(1, [reads, b"", reads.lower()]) == (2 * int(counts.sum()), 0)
        assert gpu.kset_add_rc(reads) == inv and b"closed" in lib.hypo_gpu_last_error()                     # add after a mark
        assert gpu.kset_spectrum(1).tolist() == spc.spectrum(2 * counts, 2 * counts).tolist()
        assert gpu.kset_spectrum(0).tolist() == spc.spectrum(2 * counts, zero).tolist()
    finally:
        gpu.kset_end()


CAPACITY = r"""
import numpy as np
import spectra_checker as spc
from hypo_amd import abi, capi
gpu = capi.HypoGpu(0)
rng = np.random.default_rng(78)
rnd = lambda n: bytes(rng.choice(list(b"ACGT"), n).astype(np.uint8))
k = 21
first, more = rnd(3000) + b"N" + b"AC" * 200, rnd(200000)
gpu.kset_begin(k, 1, 1 << 20)                       # 11 bytes a slot: at most 95325 slots, 47662 k-mers
gpu.kset_counts_enable(2)
gpu.kset_add(first)
keys, counts = spc.read_counts([first], k)
before = (gpu.kset_size(), gpu.kset_spectrum(0).tolist())
assert before[0][0] == keys.size and before[0][1] <= 1 << 20
assert before[1] == spc.spectrum(counts, 0 * counts).tolist() and before[1][1][0] > 2000
rc = gpu.kset_add_rc(more)                          # 199980 windows cannot fit
msg = gpu.lib.hypo_gpu_last_error().decode()
assert rc == abi.HYPO_E_CAPACITY, rc
assert str(keys.size) in msg and "GiB" in msg, msg
assert (gpu.kset_size(), gpu.kset_spectrum(0).tolist()) == before      # keys and counts are what they were
gpu.kset_add(more[:20000])                          # ... and the set still takes what fits
gpu.kset_add(first)
keys2, counts2 = spc.read_counts([first, more[:20000], first], k)
assert gpu.kset_size()[0] == keys2.size and gpu.kset_size()[1] <= 1 << 20
assert gpu.kset_spectrum(1).tolist() == spc.spectrum(counts2, 0 * counts2).tolist()
gpu.kset_end()
print("capacity ok")
"""


def test_capacity_refusal_keeps_the_counts():
    """in a process of its own, as the script of test_gpu_kset.py it restates"""
    assert "capacity ok" in tk.run_script(CAPACITY)
