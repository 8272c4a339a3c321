"""MI355X: the kernels of edit_kernel.hip on the hand-built pairs of tests/edit_cases.py — both sides of every threshold of the routing
(the exactness test of the fast band, |m - n| = 127 / 128, EDIT_LDS_STEPS, EDIT_WIDE_LDS_DIAGS, EDIT_PROBE_H, S / C / G of the wide
kernel), the densest run scripts, bytes outside ACGTN and offsets that do not start at 0.  Distance and CIGAR of every pair equal
tests/edit_checker.py, and hypo_gpu_edit_last_counts equals what tests/edit_band_model.py predicts from its traces: a pair that gives
the right answer by another way than the one it was built for fails here.  tests/test_edit_band_model_cpu.py holds the model (with
its deciding sweeps) against the checker on the same pairs.  HYPO_GPU_LIB=<path> runs the module against another build."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import edit_band_model as bm
import edit_cases as cases
import edit_checker as ec
from capi_util import ptr as _p
from hypo_amd import abi, capi

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB = os.environ.get("HYPO_GPU_LIB", capi.LIB_PATH)
OPS = "=XDI"


class Device:
    """the context, and the size of its run pool as the calls so far must have left it (hypo_gpu_init gives a fresh one: 4 runs per
    pair + 1024 at the first call, a quarter of head room on every growth, the counted size after a call that outgrew it)"""

    def __init__(self):
        self.gpu = capi.HypoGpu(0, path=LIB)
        self.pool_bytes = 0

    def grow(self, need):
        if need > self.pool_bytes:
            self.pool_bytes = need + need // 4

    def counts(self, traces, chunk_bytes=bm.CHUNK_BYTES):
        """batch_counts of the call about to be made, and the pool after it"""
        self.grow((4 * len(traces) + 1024) * 4)
        want = bm.batch_counts(traces, chunk_bytes, pool_runs=self.pool_bytes // 4)
        if want["passes"] == 2:
            self.grow(4 * want["runs"])
        return want


@pytest.fixture(scope="module")
def dev():
    return Device()


def cigars(run_off, runs, n):
    return ["".join(f"{int(r) >> 2}{OPS[int(r) & 3]}" for r in runs[int(run_off[i]):int(run_off[i + 1])]) for i in range(n)]


def assert_results(pairs, want, dist, cig):
    for i, ((a, b), (d, ops)) in enumerate(zip(pairs, want)):
        assert (int(dist[i]), cig[i]) == (d, ec.cigar(ops)), \
            f"pair {i} ({len(a)} x {len(b)}): the device has {int(dist[i])} {cig[i][:160]}, the checker {d} {ec.cigar(ops)[:160]}"


def run(dev, pairs, want, traces, chunk_bytes=bm.CHUNK_BYTES):
    predicted = dev.counts(traces, chunk_bytes)
    dist, run_off, runs = dev.gpu.edit_scripts_raw([a for a, _ in pairs], [b for _, b in pairs])
    got = dev.gpu.edit_last_counts()
    assert_results(pairs, want, dist, cigars(run_off, runs, len(pairs)))
    assert bm.counts_match(got, predicted), f"hypo_gpu_edit_last_counts {got}, the model {predicted}"
    return dist, run_off, runs, got


@pytest.mark.parametrize("name", [n for n in cases.CASES if n != "mixed_batch"])
def test_the_case_equals_the_checker_and_takes_the_model_s_routes(dev, name):
    """fast_band_edges: both outcomes of the exactness test next to either bound; delta_edges: |m - n| = 126 .. 129; k0_clamps: the band's
    placement on small and lopsided pairs; lds_edge: n + m = 509 .. 512; suffix: the trim at the ballot's edges; wide_shapes: S, C
    and G of the wide kernel; wide_values_edge: the band's values in LDS (W = 8192) and in device memory (8193 and a block pair);
    probe_edges: the probe stands up to |D| + 129; run_area: the most runs the storage has to hold; bytes_and_offsets: every byte value"""
    cases.condition(name)
    run(dev, cases.case(name), cases.expected(name), cases.traces(name))


def test_bytes_and_offsets_through_the_raw_abi(dev):
    """a_off[0] = 7, b_off[0] = 13 into buffers with other bytes in front and behind; bytes 0x00, 0x7F, 0x80, 0xFF and lower case; empty pairs"""
    pairs, want, traces = cases.case("bytes_and_offsets"), cases.expected("bytes_and_offsets"), cases.traces("bytes_and_offsets")
    n = len(pairs)
    a = np.frombuffer(b"\xAA" * cases.A_OFF0 + b"".join(p[0] for p in pairs) + b"\x55" * 9, dtype=np.uint8)
    b = np.frombuffer(b"\x00" * cases.B_OFF0 + b"".join(p[1] for p in pairs) + b"\xFF" * 5, dtype=np.uint8)
    a_off = (cases.A_OFF0 + np.concatenate([[0], np.cumsum([len(p[0]) for p in pairs])])).astype(np.uint64)
    b_off = (cases.B_OFF0 + np.concatenate([[0], np.cumsum([len(p[1]) for p in pairs])])).astype(np.uint64)
    batch = abi.EditBatch()
    batch.n_pairs, batch.a, batch.a_off, batch.b, batch.b_off = n, _p(a), _p(a_off), _p(b), _p(b_off)
    predicted = dev.counts(traces)
    dist, run_off, runs = np.zeros(n, dtype=np.uint32), np.zeros(n + 1, dtype=np.uint64), np.zeros(predicted["runs"], dtype=np.uint32)
    rc = dev.gpu.lib.hypo_gpu_edit_scripts(C.byref(batch), _p(dist), _p(run_off), _p(runs), C.c_uint64(runs.size))
    assert rc == abi.HYPO_OK, dev.gpu.lib.hypo_gpu_last_error()
    assert int(run_off[n]) == predicted["runs"]
    assert_results(pairs, want, dist, cigars(run_off, runs, n))
    assert bm.counts_match(dev.gpu.edit_last_counts(), predicted)


@pytest.mark.parametrize("shuffle", cases.MIXED_SHUFFLES)
def test_mixed_batch(dev, shuffle):
    """every case in one call among 3 000 small pairs, in two orders: the long, wide and second lists are filled by atomics in any
    order, and every result lands on its pair"""
    cases.condition("mixed_batch")
    pairs, want, traces = cases.case("mixed_batch"), cases.expected("mixed_batch"), cases.traces("mixed_batch")
    order = cases.shuffled(len(pairs), shuffle)
    run(dev, [pairs[i] for i in order], [want[i] for i in order], [traces[i] for i in order])


def test_the_lists_run_in_chunks(dev):
    """edit_chunk_mb = 1: a long list of 6 launches and a wide list of 3, one of whose pairs needs more than a chunk by itself.  The
    same results and runs as with the default chunk, byte for byte, and the launches the model's first-fit gives."""
    x = cases.text(2000, 8000)
    big = (x, cases.subs(x, 20))                                   # fast band, 256 032 bytes of move codes: 4 to a chunk
    over = cases.homo(2048, 2048)                                  # 17 groups x 4 098 anti-diagonals: more than 1 MiB
    small = cases.homo(128, 128)                                   # 8 256 bytes: 127 to a chunk
    pairs = [big] * 7 + [small] * 50 + [over] + [big] * 13 + [small] * 78
    want = [cases._align(a, b) for a, b in pairs]
    traces = [cases._model(a, b, False)[2] for a, b in pairs]
    assert traces[57]["passes"][-1]["moves_bytes"] > 1 << 20 and traces[0]["route"] == "long" and traces[7]["route"] == "lds+wide"
    one = bm.batch_counts(traces, 1 << 20, pool_runs=1 << 30)
    assert one["long"] == 21 and one["long_launches"] == 6 and one["wide"] == 129 and one["wide_launches"] == 3
    assert bm.batch_counts(traces, pool_runs=1 << 30)["long_launches"] == 1
    d0, off0, runs0, got0 = run(dev, pairs, want, traces)
    assert (got0["long_launches"], got0["wide_launches"]) == (1, 1)
    try:
        dev.gpu.set_option("edit_chunk_mb", 1)
        d1, off1, runs1, got1 = run(dev, pairs, want, traces, chunk_bytes=1 << 20)
    finally:
        dev.gpu.set_option("edit_chunk_mb", 256)
    assert (got1["long_launches"], got1["wide_launches"]) == (6, 3)
    assert np.array_equal(d0, d1) and np.array_equal(off0, off1) and np.array_equal(runs0, runs1)
    for bad in (0, 4097):
        assert dev.gpu.lib.hypo_gpu_set_option(b"edit_chunk_mb", C.c_int(bad)) == abi.HYPO_E_INVALID


def test_a_kept_results_retry_leaves_the_counts_alone(dev):
    pairs, want, traces = cases.case("delta_edges"), cases.expected("delta_edges"), cases.traces("delta_edges")
    predicted = dev.counts(traces)
    dist, run_off, runs = dev.gpu.edit_scripts_raw([a for a, _ in pairs], [b for _, b in pairs], runs_cap=0)      # HYPO_E_WORKSPACE, then the copy
    assert_results(pairs, want, dist, cigars(run_off, runs, len(pairs)))
    assert bm.counts_match(dev.gpu.edit_last_counts(), predicted)


def test_the_pool_grows_in_a_fresh_context():
    """run_area in a process of its own: more runs than the pool a context starts with, so the call passes over it twice; the second
    call finds the grown pool"""
    code = r'''
import json, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import edit_cases as cases, edit_checker as ec
from hypo_amd import capi
gpu = capi.HypoGpu(0, path=%r)
pairs, want = cases.case("run_area"), cases.expected("run_area")
assert not any(gpu.edit_last_counts().values())          # nothing computed yet
out = []
for call in range(2):
    dist, cig = gpu.edit_scripts([a for a, _ in pairs], [b for _, b in pairs])
    assert [(int(d), c) for d, c in zip(dist, cig)] == [(d, ec.cigar(ops)) for d, ops in want], call
    out.append(gpu.edit_last_counts())
print("counts " + json.dumps(out))
''' % (ROOT, HERE, LIB)
    traces = cases.traces("run_area")
    first = bm.batch_counts(traces)
    assert first["passes"] == 2 and first["runs"] > bm.fresh_pool_runs(len(traces))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "counts " in p.stdout, p.stdout[-2000:] + p.stderr[-3000:]
    got = json.loads(p.stdout.split("counts ", 1)[1])
    assert bm.counts_match(got[0], first), (got[0], first)
    assert bm.counts_match(got[1], dict(first, passes=1)), (got[1], first)
