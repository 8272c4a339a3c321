"""GPU: the records of hypo_gpu_profile_* (the kernels' own start and end times, bound to their dispatches): shape and order,
sanity against the host's clock, and that a profiled call computes what an unprofiled one does."""
import math
import time

import numpy as np
import pytest
import torch

from hypo_amd import capi, sim

pytestmark = pytest.mark.gpu

SCAN_BASES, SCAN_K = 64_000, 11


@pytest.fixture(scope="module")
def gpu():
    g = capi.HypoGpu(0)
    yield g
    g.profile_begin(0)                        # no later call of this process is profiled


@pytest.fixture(scope="module")
def work(gpu):
    """One resident POA batch and one resident scan, with what they compute unprofiled."""
    b = sim.window_batch(2000, seed=77)
    db = gpu.device_batch(b, off=b.slot_layout())
    codes, p4 = sim.random_contig(SCAN_BASES, seed=7, n_frac=0.0005)
    ds = gpu.device_scan(p4, SCAN_BASES, SCAN_K, sim.solid_bitset(codes, SCAN_K))
    gpu.profile_begin(0)
    db.run()
    ds.run()
    poa = [x.copy() for x in db.results()]
    scan = [np.array(x).copy() for x in ds.results()]
    return db, ds, poa, scan


def _same_poa(got, want):
    bases, off, ln, st = got
    wb, _, wln, wst = want
    if not ((st == wst).all() and (ln == wln).all()):
        return False
    return all((bases[int(o):int(o) + int(l)] == wb[int(o):int(o) + int(l)]).all() for o, l in zip(off[:-1], ln))


def test_record_shapes_and_bounds(gpu, work):
    db, ds, _, _ = work
    torch.cuda.synchronize()
    gpu.profile_begin(2)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    db.run()
    torch.cuda.synchronize()
    wall_ms = (time.perf_counter() - t0) * 1e3
    ds.run()
    torch.cuda.synchronize()
    prof = gpu.profile_read()
    gpu.profile_begin(0)
    assert [len(p) for p in prof] == [8, 3]
    poa, scan = prof
    print("poa record", poa, "wall", wall_ms, "scan record", scan)
    assert all(math.isfinite(v) and v >= 0.0 for v in poa + scan)
    assert all(v <= poa[7] for v in poa[1:7])             # every class inside the whole call
    assert poa[0] <= poa[7]
    assert poa[7] <= wall_ms                              # the device's interval lies inside the host's
    assert poa[7] > 0.0 and poa[0] > 0.0 and scan[0] > 0.0
    assert scan[1] == 0.0 and scan[2] == 0.0


def test_profiled_calls_compute_the_same(gpu, work):
    db, ds, poa_want, scan_want = work
    gpu.profile_begin(4)
    db.run()
    ds.run()
    poa_on = db.results()
    scan_on = ds.results()
    assert len(gpu.profile_read()) == 2
    gpu.profile_begin(0)
    db.run()
    ds.run()
    poa_off = db.results()
    scan_off = ds.results()
    for got in (poa_on, poa_off):
        assert _same_poa(got, poa_want)
    for got in (scan_on, scan_off):
        assert got[3] == scan_want[3]
        for a, w in zip(got[:3], scan_want[:3]):
            assert a.tobytes() == w.tobytes()


def test_only_armed_calls_are_recorded(gpu, work):
    db, _, poa_want, _ = work
    gpu.profile_begin(1)
    for _ in range(3):
        db.run()
    torch.cuda.synchronize()
    prof = gpu.profile_read()
    gpu.profile_begin(0)
    assert [len(p) for p in prof] == [8]
    assert _same_poa(db.results(), poa_want)
