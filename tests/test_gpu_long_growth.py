"""MI355X: LONG windows whose consensus outgrows (or undercuts) the draft (tests/long_growth.py) through the default dispatch of
hypo_gpu_poa_batch, against the oracle and — where oracle/_ref travelled — the real reference; the giant family in size class 6, with
the arena it needs and with one that is too small; and the whole bounded LONG space of tests/exhaustive_parity.py against the oracle.
The CPU half (emulator, every class on its own, ASan) is tests/test_long_growth_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import exhaustive_parity as ex
import long_growth as lg
from hypo_amd import abi, capi
from hypo_amd.batch import build_batch

pytestmark = pytest.mark.gpu

# family: (seed, windows before the N twins) ...: 5 708 windows
PLAN = {
    "own_ins": [(1, 400), (2, 400)],
    "shared_ins": [(1, 75), (2, 75)],
    "stacked": [(1, 300), (2, 300)],
    "shrink": [(1, 400), (2, 400)],
    "prefix_suffix": [(1, 250), (2, 250)],
    "giant": [(1, 2), (2, 2)],
}


@pytest.fixture(scope="module")
def gpu():
    import os
    return capi.HypoGpu(0, path=os.environ["HYPO_GPU_LIB"]) if os.environ.get("HYPO_GPU_LIB") else capi.HypoGpu(0)


def _texts(bases, off, ln, n):
    return [bases[int(off[i]):int(off[i]) + int(ln[i])].tobytes() for i in range(n)]


def test_the_plan_holds_5000_windows():
    assert sum(2 * n for plan in PLAN.values() for _, n in plan) >= 5000


@pytest.mark.parametrize("family", lg.FAMILIES)
def test_family_vs_oracle_and_real_reference(gpu, oracle_lib, family):
    import oracle
    ws = [w for seed, n in PLAN[family] for w in lg.windows(family, seed, n)]
    b = build_batch(ws)
    off = b.slot_layout()
    bases, _, ln, st = gpu.poa_batch(b, off=off)
    s = gpu.last_stats()
    ob, _, oln, ost, cells, aligns = oracle_lib.poa_batch_raw(b, off=off)
    assert (ost == 0).all()
    got, want = _texts(bases, off, ln, len(ws)), _texts(ob, off, oln, len(ws))
    bad = [i for i in range(len(ws)) if st[i] != abi.ST_OK or got[i] != want[i]]
    assert not bad, (f"{family}: {len(bad)} of {len(ws)} windows; first: window {bad[0]}, draft {len(ws[bad[0]].draft)}, arms "
                     f"{[len(a) for a in ws[bad[0]].internal + ws[bad[0]].prefix + ws[bad[0]].suffix]}: status {int(st[bad[0]])}, "
                     f"{int(ln[bad[0]])} bases, oracle {int(oln[bad[0]])}")
    assert s["n_failed"] == 0 and s["dp_cells"] == cells and s["n_alignments"] == aligns
    line = f"{family}: {len(ws)} windows, ran in classes 0-6: {list(s['n_class'][:7])}"
    if family == "giant":
        assert s["n_class"][6] == len(ws), s["n_class"]          # they really ran in class 6, and were answered
    if oracle.Ref.available():
        rb, _, rln, rst, _ = oracle.Ref().poa_batch_raw(b, off=off)
        filtered = rst == oracle.REF_ST_FILTERED
        line += f"; FILTERED by the reference's own Window: {int(filtered.sum())} ({100 * filtered.mean():.2f} %)"
        print(line)
        assert filtered.mean() <= 0.05
        ref = _texts(rb, off, rln, len(ws))
        assert [i for i in np.nonzero(~filtered)[0] if rst[i] != 0 or ref[i] != got[i]] == []
    else:
        print(line)


def test_an_arena_that_is_too_small_answers_capacity_never_other_bytes(gpu, oracle_lib):
    """The giant family and full-size shared_ins windows with an 8 MB arena (two slices of 4 MB): what class 6 can no longer hold comes
    back HYPO_ST_CAPACITY, everything else with the oracle's bytes."""
    ws = lg.windows("giant", 1, 2) + lg.windows("shared_ins", 3, 20)
    b = build_batch(ws)
    off = b.slot_layout()
    ob, _, oln, ost, _, _ = oracle_lib.poa_batch_raw(b, off=off)
    want = _texts(ob, off, oln, len(ws))
    assert gpu.lib.hypo_gpu_set_option(b"giant_arena_mb", C.c_int(8)) == 0
    try:
        g2 = type(gpu)(0)                                        # (re-initialises the library's context: its POA state is created anew)
        bases, _, ln, st = g2.poa_batch(b, off=off)
        s = g2.last_stats()
    finally:
        assert gpu.lib.hypo_gpu_set_option(b"giant_arena_mb", C.c_int(1024)) == 0
        type(gpu)(0)
    got = _texts(bases, off, ln, len(ws))
    for i in range(len(ws)):
        assert st[i] in (abi.ST_OK, abi.ST_CAPACITY), (i, int(st[i]))
        assert st[i] != abi.ST_OK or got[i] == want[i], i
    n_cap = int((st == abi.ST_CAPACITY).sum())
    assert (st[:4] == abi.ST_CAPACITY).all() and s["n_failed"] == n_cap and n_cap < len(ws), (st, s)
    # and the same context answers all of them once it has its arena again
    bases, _, ln, st = gpu.poa_batch(b, off=off)
    assert (st == 0).all() and _texts(bases, off, ln, len(ws)) == want


def test_bounded_long_space_vs_oracle(gpu, oracle_lib):
    """Every window of exhaustive_parity.LONG_SPACES["l2n3"] (8 937 300: alphabet {A, C}, drafts of 1-4, 3 arms of 0-4 bases, every kind
    multiset) under the default long-read scores and one alternative, default dispatch, against the oracle."""
    n = 0
    for b in ex.chunks("l2n3", 1_000_000):
        off = b.slot_layout()
        db = gpu.device_batch(b, off=off)
        for sc in ex.LONG_SCORE_SETS:
            ob, _, oln, ost = oracle_lib.poa_batch_raw(b, scores=sc, off=off)[:4]
            db.run(scores=sc)
            gb, _, gln, gst = db.results()
            w = ex.first_difference((gb, gln, gst), (ob, oln, ost), off)
            assert w < 0, (f"scores {sc}: {ex.describe(b, w)}: device status {int(gst[w])} "
                           f"{gb[int(off[w]):int(off[w]) + int(gln[w])].tobytes()!r}, oracle status {int(ost[w])} {ob[int(off[w]):int(off[w]) + int(oln[w])].tobytes()!r}")
        del db
        n += b.n_windows
    assert n == ex.space_size("l2n3")
