"""GPU: hypo_gpu_edit_scripts (edit_kernel.hip) against the numpy restatement of the canonical alignment (tests/edit_checker.py):
distance and CIGAR of every pair, exactly, on the fast path, the long (scratch) form of it and the wide path."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import edit_checker as ec

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def gpu():
    from hypo_amd import capi
    return capi.HypoGpu(0)


def mutate(rnd, s, rate, alpha="ACGT"):
    out, i = [], 0
    while i < len(s):
        r = rnd.random()
        if r < rate / 3:
            out.append(rnd.choice(alpha))
            i += 1
        elif r < 2 * rate / 3:
            i += 1
        elif r < rate:
            out.append(rnd.choice(alpha))
        else:
            out.append(s[i])
            i += 1
    return "".join(out)


def check(gpu, pairs):
    a = [p[0].encode() for p in pairs]
    b = [p[1].encode() for p in pairs]
    dist, cig = gpu.edit_scripts(a, b)
    for i, (x, y) in enumerate(zip(a, b)):
        d, ops = ec.align(x, y)
        assert (int(dist[i]), cig[i]) == (d, ec.cigar(ops)), f"pair {i}: {len(x)} x {len(y)}: {int(dist[i])} {cig[i][:200]} vs {d} {ec.cigar(ops)[:200]}"
    return dist, cig


def test_random_pairs_short(gpu):
    rnd = random.Random(1)
    pairs = []
    for _ in range(1500):
        a = "".join(rnd.choice("ACGTN" if rnd.random() < 0.1 else "ACGT") for _ in range(rnd.randint(0, 300)))
        pairs.append((a, mutate(rnd, a, rnd.choice([0, 0.01, 0.05, 0.1, 0.2, 0.3]))))
    check(gpu, pairs)


def test_equal_and_empty_sides(gpu):
    rnd = random.Random(2)
    s = "".join(rnd.choice("ACGT") for _ in range(700))
    pairs = [("", ""), ("A", "A"), (s, s), ("", s[:50]), (s[:60], ""), ("", s), (s, ""), ("ACGT", "ACGT" * 3), ("AC" * 40, "")]
    dist, cig = check(gpu, pairs)
    assert cig[0] == "" and cig[2] == "700=" and cig[3] == "50I" and cig[4] == "60D"


def test_homopolymers_and_tandem_repeats(gpu):
    rnd = random.Random(3)
    pairs = []
    for _ in range(400):
        unit = "".join(rnd.choice("ACGT") for _ in range(rnd.randint(1, 4)))
        core = unit * rnd.randint(1, 60)
        pre = "".join(rnd.choice("ACGT") for _ in range(rnd.randint(0, 10)))
        suf = "".join(rnd.choice("ACGT") for _ in range(rnd.randint(0, 10)))
        a = pre + core + suf
        b = pre + unit * rnd.randint(0, 70) + suf
        if rnd.random() < 0.5:
            b = mutate(rnd, b, 0.05)
        pairs.append((a, b))
    check(gpu, pairs)


def test_long_and_wide_pairs(gpu):
    """2-8 kbp: distance > 64 or |m - n| > 64 take the wide path; low-divergence ones the fast path with moves in the scratch"""
    rnd = random.Random(4)
    pairs = []
    for n in (2000, 3500, 5000, 8000):
        a = "".join(rnd.choice("ACGT") for _ in range(n))
        pairs.append((a, mutate(rnd, a, 0.01)))                 # fast band, moves in the scratch
        pairs.append((a, mutate(rnd, a, 0.15)))                 # distance far beyond the band
        pairs.append((a, a[: n // 2] + a[n // 2 + 300:]))        # |delta| = 300
        pairs.append((a, a[:100] + "T" * 400 + a[100:]))
        pairs.append((a, mutate(rnd, a[:n // 3] + a[n // 3 + 400:], 0.05)))   # |delta| > 127 and a probe band too narrow: second pass
    pairs.append(("A" * 4000, "A" * 3700 + "C" * 10))            # a homopolymer LONG window
    pairs.append(("A" * 4200, "A" * 4000))
    pairs.append(("ACGT" * 500, "TGCA" * 600))
    check(gpu, pairs)


def test_wide_band_beyond_lds(gpu):
    """two unrelated ~18 kbp sequences (|m - n| = 200): the probe is not exact, the second pass needs a band of more than
    EDIT_WIDE_LDS_DIAGS = 8192 diagonals, whose values live in the scratch instead of LDS"""
    rnd = random.Random(8)
    a = "".join(rnd.choice("ACGT") for _ in range(18000))
    b = "".join(rnd.choice("ACGT") for _ in range(17800))
    d, ops = ec.align(a.encode(), b.encode())
    assert d > 8400                      # band = [min(0,D) - h, max(0,D) + h], h = (d - 200) / 2: more than 8192 diagonals
    dist, cig = gpu.edit_scripts([a, "ACGT"], [b, "AGT"])
    assert (int(dist[0]), cig[0]) == (d, ec.cigar(ops))
    d1, ops1 = ec.align(b"ACGT", b"AGT")
    assert (int(dist[1]), cig[1]) == (d1, ec.cigar(ops1))


def test_million_small_pairs_and_repeated_calls(gpu):
    rnd = np.random.default_rng(5)
    n = 1_000_000
    lens = rnd.integers(0, 24, n)
    alpha = np.frombuffer(b"ACGT", dtype=np.uint8)
    a_all = alpha[rnd.integers(0, 4, int(lens.sum()))].tobytes()
    off = np.concatenate([[0], np.cumsum(lens)])
    a = [a_all[off[i]:off[i + 1]] for i in range(n)]
    b = list(a)
    pick = rnd.choice(n, n // 3, replace=False)
    for i in pick:
        s = bytearray(b[i])
        pos = int(rnd.integers(0, len(s) + 1))
        s[pos:pos] = b"G" * int(rnd.integers(1, 3))
        b[i] = bytes(s)
    dist, cig = gpu.edit_scripts(a, b)
    sample = rnd.choice(n, 4000, replace=False)
    for i in sample:
        d, ops = ec.align(a[i], b[i])
        assert (int(dist[i]), cig[i]) == (d, ec.cigar(ops)), i
    assert int(dist.sum()) == int(sum(len(b[i]) - len(a[i]) for i in pick))
    for rep in range(20):                                      # many calls in a row, different sizes (scratch re-used / grown)
        m = 1 + rep * 97
        d2, c2 = gpu.edit_scripts(a[:m], b[:m])
        assert np.array_equal(d2, dist[:m]) and c2 == cig[:m]


def test_workspace_retry(gpu):
    rnd = random.Random(6)
    a = ["".join(rnd.choice("ACGT") for _ in range(200)) for _ in range(50)]
    b = [mutate(rnd, x, 0.2) for x in a]
    from hypo_amd import abi
    d0, off0, runs0 = gpu.edit_scripts_raw(a, b)
    d1, off1, runs1 = gpu.edit_scripts_raw(a, b, runs_cap=0)        # HYPO_E_WORKSPACE first, then the size it reported
    assert np.array_equal(d0, d1) and np.array_equal(off0, off1) and np.array_equal(runs0, runs1)
    assert int(off0[-1]) > 4 * 50 + 16             # (the default first capacity was too small as well)
    import ctypes as C
    batch = abi.EditBatch()
    aa = np.frombuffer("".join(a).encode(), dtype=np.uint8)
    bb = np.frombuffer("".join(b).encode(), dtype=np.uint8)
    ao = np.concatenate([[0], np.cumsum([len(x) for x in a])]).astype(np.uint64)
    bo = np.concatenate([[0], np.cumsum([len(x) for x in b])]).astype(np.uint64)
    batch.n_pairs, batch.a, batch.a_off, batch.b, batch.b_off = 50, aa.ctypes.data, ao.ctypes.data, bb.ctypes.data, bo.ctypes.data
    dist = np.zeros(50, dtype=np.uint32)
    ro = np.zeros(51, dtype=np.uint64)
    rc = gpu.lib.hypo_gpu_edit_scripts(C.byref(batch), dist.ctypes.data_as(C.c_void_p), ro.ctypes.data_as(C.c_void_p), None, C.c_uint64(0))
    assert rc == abi.HYPO_E_WORKSPACE and np.array_equal(ro, off0) and np.array_equal(dist, d0)


def test_workspace_retry_copies_the_kept_results(gpu):
    """after HYPO_E_WORKSPACE the context keeps the call's results: the retry naming the same batch copies them out without
    computing again (shown by changing the bytes in between, which the contract forbids); a call after that computes afresh"""
    import ctypes as C
    from hypo_amd import abi
    a = [b"ACGTACGTAC" * 20, b"TTTTGGGGCCCCAAAA" * 5]
    b = [b"ACGTACCTAC" * 20, b"TTTTGGGCCCCAAAAA" * 5]
    aa = np.frombuffer(b"".join(a), dtype=np.uint8).copy()
    bb = np.frombuffer(b"".join(b), dtype=np.uint8).copy()
    ao = np.array([0, len(a[0]), len(a[0]) + len(a[1])], dtype=np.uint64)
    bo = np.array([0, len(b[0]), len(b[0]) + len(b[1])], dtype=np.uint64)
    batch = abi.EditBatch()
    batch.n_pairs, batch.a, batch.a_off, batch.b, batch.b_off = 2, aa.ctypes.data, ao.ctypes.data, bb.ctypes.data, bo.ctypes.data
    dist = np.zeros(2, dtype=np.uint32)
    ro = np.zeros(3, dtype=np.uint64)
    P = lambda x: x.ctypes.data_as(C.c_void_p)
    assert gpu.lib.hypo_gpu_edit_scripts(C.byref(batch), P(dist), P(ro), None, C.c_uint64(0)) == abi.HYPO_E_WORKSPACE
    want = [ec.align(x, y) for x, y in zip(a, b)]
    assert list(dist) == [w[0] for w in want]
    bb[:] = ord("A")                                        # (bytes changed: a fresh computation would now differ)
    runs = np.zeros(int(ro[-1]), dtype=np.uint32)
    assert gpu.lib.hypo_gpu_edit_scripts(C.byref(batch), P(dist), P(ro), P(runs), C.c_uint64(runs.size)) == 0
    ops = "=XDI"
    got = ["".join(f"{int(r) >> 2}{ops[int(r) & 3]}" for r in runs[int(ro[i]):int(ro[i + 1])]) for i in range(2)]
    assert got == [ec.cigar(w[1]) for w in want] and list(dist) == [w[0] for w in want]
    runs2 = np.zeros(1024, dtype=np.uint32)
    assert gpu.lib.hypo_gpu_edit_scripts(C.byref(batch), P(dist), P(ro), P(runs2), C.c_uint64(runs2.size)) == 0
    assert list(dist) == [ec.align(x, bytes(bb[int(bo[i]):int(bo[i + 1])]))[0] for i, x in enumerate(a)]


def test_two_contexts_on_one_device():
    code = r'''
import sys, threading, random
sys.path.insert(0, %r); sys.path.insert(0, %r)
import edit_checker as ec
from hypo_amd import capi
gpu = capi.HypoGpu(0, devices=[0, 0])
assert gpu.lib.hypo_gpu_num_devices() == 2
res, errs = {}, []
def work(slot):
    try:
        assert gpu.lib.hypo_gpu_use_device(slot) == 0
        rnd = random.Random(slot)
        a = ["".join(rnd.choice("ACGT") for _ in range(rnd.randint(0, 400))) for _ in range(3000)]
        b = ["".join(c for c in x if rnd.random() > 0.05) for x in a]
        for _ in range(3):
            d, cg = gpu.edit_scripts([x.encode() for x in a], [y.encode() for y in b])
        for i in range(0, 3000, 7):
            dd, ops = ec.align(a[i].encode(), b[i].encode())
            assert (int(d[i]), cg[i]) == (dd, ec.cigar(ops))
        res[slot] = True
    except Exception as e:
        errs.append(repr(e))
th = [threading.Thread(target=work, args=(s,)) for s in (0, 1)]
[t.start() for t in th]; [t.join() for t in th]
assert not errs and len(res) == 2, errs
print("ok")
''' % (ROOT, HERE)
    env = dict(os.environ, HYPO_ALLOW_DUP_DEVICES="1")
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "ok" in p.stdout, p.stdout[-2000:] + p.stderr[-3000:]
