"""GPU: the exact k-mer set of C-ABI 11 (kset_kernel.hip) against the CPU checker (tests/qv_checker.py), as exact integers."""
import os
import subprocess
import sys

import numpy as np
import pytest

import qv_checker as qc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
KS = [12, 15, 16, 21, 22, 31]
COMP = bytes.maketrans(b"ACGT", b"TGCA")


@pytest.fixture(scope="module")
def gpu():
    from hypo_amd import capi
    return capi.HypoGpu(0)


def rnd(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(list(alphabet), n).astype(np.uint8))


def mutate(rng, s, rate):
    a = bytearray(s)
    for p in np.flatnonzero(rng.random(len(a)) < rate):
        a[p] = b"ACGT"[(b"ACGT".index(a[p]) + 1 + int(rng.integers(3))) % 4] if a[p] in b"ACGT" else a[p]
    return bytes(a)


def palindrome(k):
    half = b"ACGTTGCAAGCTTAGG"[:k // 2]
    return half + half.translate(COMP)[::-1]


def read_records(rng, k, genome_len=20000, cov=30, read_len=150):
    """reads of a random genome with errors, both strands, then every oddity of tests/test_qv_checker_cpu.py"""
    genome = rnd(rng, genome_len)
    recs = []
    for _ in range(genome_len * cov // read_len):
        p = int(rng.integers(0, genome_len - read_len))
        r = mutate(rng, genome[p:p + read_len], 0.01)
        recs.append(r.translate(COMP)[::-1] if rng.random() < 0.5 else r)
    recs += [rnd(rng, 60, b"ACGTN"), rnd(rng, 70, b"ACGTRYKM"), rnd(rng, 90).lower(), rnd(rng, 50, b"ACGTacgtn")]
    recs += [rnd(rng, k - 1), rnd(rng, k), b"", b"N" * 40, b"A" * 50, b"AC" * 30, rnd(rng, k - 1) + b"N" + rnd(rng, k - 1)]
    if k % 2 == 0:
        recs += [palindrome(k), b"G" * 5 + palindrome(k).lower() + b"T" * 5]
    return genome, recs


def queries(rng, k, genome, recs):
    return [genome, mutate(rng, genome, 0.002), rnd(rng, 5000), rnd(rng, k - 1), b"", rnd(rng, k), mutate(rng, recs[0], 0.05), recs[1],
            b"acgtn" * 20, b"", b"", rnd(rng, 3), b"T" * 100, b"GT" * 50, rnd(rng, 9000, b"ACGTN"), mutate(rng, recs[2], 0.1).lower(),
            genome[:8192 - 5], genome[:40], genome[100:8300]] + [mutate(rng, r, 0.02) for r in recs[3:200]]


def check_queries(gpu, qs, k, R):
    total, missing = gpu.kset_query(qs)
    want = [qc.seq_stats(q, k, R) for q in qs]
    assert [(int(t), int(m)) for t, m in zip(total, missing)] == want


def decode(codes, k):
    """the k-mers of `codes` as one byte string, an N between two of them"""
    out = np.full((codes.size, k + 1), ord("N"), dtype=np.uint8)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    for j in range(k):
        out[:, j] = lut[((codes >> np.uint64(2 * (k - 1 - j))) & np.uint64(3)).astype(np.int64)]
    return out


@pytest.mark.parametrize("k", KS)
def test_set_equals_checker(gpu, k):
    rng = np.random.default_rng(1000 + k)
    genome, recs = read_records(rng, k)
    R = qc.read_set(recs, k)
    assert R.size > 20000
    blob = b"\n".join(recs)
    qs = queries(rng, k, genome, recs)
    # one large add
    gpu.kset_begin(k, R.size)
    try:
        gpu.kset_add(blob)
        n, table_bytes = gpu.kset_size()
        assert n == R.size and table_bytes >= 2 * 8 * n                  # (the load stays at or below one half)
        check_queries(gpu, qs, k, R)
        # every k-mer of the set, as sequences: nothing is missing
        text = decode(R, k)
        total, missing = gpu.kset_query([text.tobytes()])
        assert (int(total[0]), int(missing[0])) == (R.size, 0)
        some = [text[i, :k].tobytes() for i in range(0, R.size, max(1, R.size // 300))]
        total, missing = gpu.kset_query(some + [s.translate(COMP)[::-1] for s in some])
        assert total.tolist() == [1] * (2 * len(some)) and missing.tolist() == [0] * (2 * len(some))
        # the same bytes again add nothing (the table may grow: room for a call's worst case is made before the call)
        gpu.kset_add(blob)
        assert gpu.kset_size()[0] == n and gpu.kset_size()[1] >= table_bytes
        check_queries(gpu, qs[:6], k, R)
    finally:
        gpu.kset_end()
    # the same bytes in many small overlapping adds into a table that starts at its smallest: it grows, the set is the same
    gpu.kset_begin(k, 1)
    try:
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
        assert gpu.kset_size()[0] == R.size
        check_queries(gpu, qs, k, R)
    finally:
        gpu.kset_end()


@pytest.mark.parametrize("k", [12, 21, 22, 31])
def test_contention(gpu, k):
    """poly-A, poly-AC and a million copies of one read: every lane of many waves at the same few slots"""
    rng = np.random.default_rng(k)
    hot = rnd(rng, 150)
    parts = [b"A" * 200000, b"AC" * 100000, hot, rnd(rng, 300)]
    R = qc.read_set(parts, k)
    blob = b"\n".join(parts[:2]) + b"\n" + (hot + b"\n") * 10 ** 6 + parts[3]
    gpu.kset_begin(k, 1)
    try:
        gpu.kset_add(blob)
        assert gpu.kset_size()[0] == R.size
        qs = [b"A" * 1000, b"T" * 1000, b"CA" * 500, b"GT" * 77, hot, mutate(rng, hot, 0.05), parts[3], rnd(rng, 2000), hot * 50]
        check_queries(gpu, qs, k, R)
    finally:
        gpu.kset_end()


def test_argument_errors(gpu):
    from hypo_amd import abi
    import ctypes as C
    lib = gpu.lib
    n = C.c_uint64(0)
    one = np.zeros(1, dtype=np.uint64)
    off = np.array([0, 4], dtype=np.uint64)
    assert lib.hypo_gpu_kset_add(b"ACGT" * 10, C.c_uint64(40)) == abi.HYPO_E_INVALID            # no begin
    assert lib.hypo_gpu_kset_size(C.byref(n), None) == abi.HYPO_E_INVALID
    assert lib.hypo_gpu_kset_query(b"ACGT", off.ctypes.data_as(C.c_void_p), C.c_uint32(1), one.ctypes.data_as(C.c_void_p),
                                   one.ctypes.data_as(C.c_void_p)) == abi.HYPO_E_INVALID
    for k in (0, 11, 32, 64):
        assert lib.hypo_gpu_kset_begin(C.c_uint32(k), C.c_uint64(10), C.c_uint64(0)) == abi.HYPO_E_INVALID
        assert b"12..31" in lib.hypo_gpu_last_error()
    assert lib.hypo_gpu_kset_size(C.byref(n), None) == abi.HYPO_E_INVALID                        # a refused begin opens nothing
    gpu.kset_begin(12, 10)
    try:
        bad = np.array([0, 4, 2], dtype=np.uint64)
        two = np.zeros(2, dtype=np.uint64)
        assert lib.hypo_gpu_kset_query(b"ACGT", bad.ctypes.data_as(C.c_void_p), C.c_uint32(2), two.ctypes.data_as(C.c_void_p),
                                       two.ctypes.data_as(C.c_void_p)) == abi.HYPO_E_INVALID
        assert gpu.kset_size()[0] == 0
        total, missing = gpu.kset_query([b"ACGTACGTACGTACGT"])
        assert (int(total[0]), int(missing[0])) == (5, 5)                 # an empty set lacks everything
    finally:
        gpu.kset_end()
    assert lib.hypo_gpu_kset_end() == 0                                   # ending twice is harmless


def run_script(code, env_extra=None, timeout=600):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + HERE + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.update(env_extra or {})
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    return p.stdout


CAPACITY = r"""
import time
import numpy as np
import qv_checker as qc
from hypo_amd import abi, capi
gpu = capi.HypoGpu(0)
rng = np.random.default_rng(77)
rnd = lambda n: bytes(rng.choice(list(b"ACGT"), n).astype(np.uint8))
k = 21
first, more = rnd(3000), rnd(200000)
qs = [first, more[:5000], rnd(1000), b""]
gpu.kset_begin(k, 1, 1 << 20)                       # at most 131072 slots: 65536 k-mers
gpu.kset_add(first)
R = qc.read_set([first], k)
before = (gpu.kset_size(), [x.tolist() for x in gpu.kset_query(qs)])
assert before[0][0] == R.size and before[1] == [[qc.seq_stats(q, k, R)[i] for q in qs] for i in (0, 1)]
t0 = time.time()
rc = gpu.kset_add_rc(more)                          # 199980 windows cannot fit
dt = time.time() - t0
msg = gpu.lib.hypo_gpu_last_error().decode()
print("rc", rc, "seconds", round(dt, 3), msg)
assert rc == abi.HYPO_E_CAPACITY, rc
assert dt < 30, dt
assert str(R.size) in msg and "GiB" in msg, msg     # names the size reached
after = (gpu.kset_size(), [x.tolist() for x in gpu.kset_query(qs)])
assert after == before                              # the set is what it was before the call
gpu.kset_add(more[:20000])                          # ... and still takes what fits
R2 = qc.read_set([first, more[:20000]], k)
assert gpu.kset_size()[0] == R2.size
assert [x.tolist() for x in gpu.kset_query(qs)] == [[qc.seq_stats(q, k, R2)[i] for q in qs] for i in (0, 1)]
gpu.kset_end()
# the context runs a normal cycle afterwards
gpu.kset_begin(16, 1000)
gpu.kset_add(more)
R3 = qc.read_set([more], 16)
assert gpu.kset_size()[0] == R3.size
assert [x.tolist() for x in gpu.kset_query(qs)] == [[qc.seq_stats(q, 16, R3)[i] for q in qs] for i in (0, 1)]
gpu.kset_end()
print("capacity ok")
"""


def test_capacity_is_an_answer():
    """a max_bytes the set outgrows: HYPO_E_CAPACITY at once, the set unchanged, the context usable (in a process of its own, whose
    time limit is there for accidents only)"""
    out = run_script(CAPACITY)
    assert "capacity ok" in out, out


TWO_CONTEXTS = r"""
import numpy as np
import qv_checker as qc
from hypo_amd import capi
gpu = capi.HypoGpu(devices=[0, 0])
rng = np.random.default_rng(5)
rnd = lambda n: bytes(rng.choice(list(b"ACGT"), n).astype(np.uint8))
a, b = rnd(50000), rnd(30000)
qs = [a[:3000], b[:3000], rnd(500)]
gpu.use_device(0); gpu.kset_begin(21, 1000); gpu.kset_add(a)
gpu.use_device(1); gpu.kset_begin(15, 1000); gpu.kset_add(b)
Ra, Rb = qc.read_set([a], 21), qc.read_set([b], 15)
for slot, k, R in ((0, 21, Ra), (1, 15, Rb), (0, 21, Ra)):
    gpu.use_device(slot)
    assert gpu.kset_size()[0] == R.size
    assert [x.tolist() for x in gpu.kset_query(qs)] == [[qc.seq_stats(q, k, R)[i] for q in qs] for i in (0, 1)]
gpu.use_device(1); gpu.kset_end()
gpu.use_device(0)
assert gpu.kset_size()[0] == Ra.size
gpu.kset_end()
print("two contexts ok")
"""


def test_two_contexts_hold_different_sets():
    out = run_script(TWO_CONTEXTS, {"HYPO_ALLOW_DUP_DEVICES": "1"})
    assert "two contexts ok" in out, out
