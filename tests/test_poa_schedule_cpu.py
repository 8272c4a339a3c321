"""The host side of poa_run as data (hypo_amd/csrc/poa_sched.hpp), pinned without a GPU through tests/emu/sched_cases.cpp:
workspace layout, history, schedule, grid sizes.  The expected values restate what poa_run computed inline before the scheduler
was separated from the code that enqueues; the knobs are read from the environment, as poa_run reads them."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from hypo_amd import capi

HERE = os.path.dirname(os.path.abspath(__file__))
N_C2 = 97078                      # the C2 batch: 59780 + 20392 + 16906 windows in classes 0 - 2
KNOBS = ("CLASS0", "SEQUENTIAL", "SYNC_PLAN", "CAPS", "ORDER", "POLL", "POLL_WAVES", "ADAPT", "ADAPT_LOG", "WAVES_PER_CU")


class Pinned(C.Structure):
    _fields_ = [("plan", C.c_uint32 * 8), ("final_count", C.c_uint32 * 8), ("unused", C.c_uint32 * 8), ("work", C.c_uint64 * 8)]


class History(C.Structure):
    _fields_ = [("planned", C.c_uint32 * 8), ("last_count", C.c_uint32 * 8), ("last_planned", C.c_uint32 * 8),
                ("work", C.c_uint64 * 3), ("measured_gw", C.c_uint64), ("valid", C.c_bool)]


class Schedule(C.Structure):
    _fields_ = [("sequential", C.c_bool), ("four_groups", C.c_bool), ("caps", C.c_int * 3), ("order", C.c_char * 4),
                ("long_first_pass", C.c_bool), ("first4", C.c_uint32), ("poll_waves", C.c_uint32), ("poll_cap", C.c_int),
                ("hint3", C.c_uint32), ("hint4", C.c_uint32), ("hint5", C.c_uint32), ("mopup4", C.c_uint32)]


class Layout(C.Structure):
    _fields_ = [("queues", C.c_size_t), ("keys", C.c_size_t), ("carry", C.c_size_t), ("spill", C.c_size_t), ("dirg3", C.c_size_t),
                ("scratch", C.c_size_t), ("spill_bytes", C.c_size_t), ("groups3", C.c_int), ("prefix", C.c_size_t)]


# footprints {lds, vgprs, max_waves} of class 0 with four groups per wave, with two, and of classes 1, 2, 3 (made up, near the product's)
FP = ((15872, 96, 10), (8192, 96, 10), (8192, 128, 8), (14848, 128, 8), (16384, 128, 8))


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "emu"), "sched"])
    lib = C.CDLL(os.path.join(HERE, "_build", os.environ.get("HYPO_SCHED_LIB", "libhypo_sched.so")))
    sizes = (C.c_uint64 * 4)()
    lib.sched_sizes(sizes)
    assert list(sizes) == [C.sizeof(History), C.sizeof(Schedule), C.sizeof(Pinned), C.sizeof(Layout)]
    lib.sched_grid.restype = C.c_long
    lib.sched_late_arrivals.restype = lib.sched_rare_grid_hint.restype = C.c_uint32
    return lib


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv("HYPO_POA_" + k, raising=False)


def history(valid=True, planned=(59780, 20392, 16906), last_count=None, last_planned=None, work=(0, 0, 0), gw=32):
    h = History()
    for name, v in (("planned", planned), ("last_count", last_count if last_count is not None else planned),
                    ("last_planned", last_planned if last_planned is not None else planned)):
        for c, x in enumerate(v):
            getattr(h, name)[c] = x
    for c in range(3):
        h.work[c] = work[c]
    h.measured_gw, h.valid = gw, valid
    return h


def schedule(lib, h, n=N_C2, groups4=2048, fp=FP):
    s = Schedule()
    flat = (C.c_int64 * 15)(*[x for f in fp for x in f])
    lib.sched_schedule(C.byref(h), C.c_uint32(n), C.c_int(groups4), flat, C.byref(s))
    return s


def class3(planned3, arrivals):
    """history of a C2-sized call whose plan holds planned3 windows in class 3 and whose predecessor saw `arrivals` more arrive late"""
    return history(planned=(59780, 20392, 16906, planned3), last_count=(59780, 20392, 16906, planned3 + arrivals))


@pytest.mark.parametrize("planned3,arrivals,waves,cap", [
    (0, 0, 0, None), (0, 40, 8, 1), (0, 514, 64, 1), (0, 1024, 128, 1), (0, 1025, 256, 1), (0, 2048, 512, 1), (0, 2049, 2561, 2),
    (0, 3033, 3791, 2), (0, 3034, 0, None),             # (more than 1/32 of the batch is late: no polling launch)
    (1107, 0, 1383, 2), (1107, 3034, 0, None)])
def test_poll_sizing(lib, planned3, arrivals, waves, cap):
    s = schedule(lib, class3(planned3, arrivals))
    assert not s.sequential and s.poll_waves == waves
    if cap is not None:
        assert s.poll_cap == cap


def test_poll_knobs(lib, monkeypatch):
    monkeypatch.setenv("HYPO_POA_POLL", "0")
    assert schedule(lib, class3(0, 514)).poll_waves == 0
    monkeypatch.delenv("HYPO_POA_POLL")
    monkeypatch.setenv("HYPO_POA_POLL_WAVES", "77")
    assert schedule(lib, class3(0, 514)).poll_waves == 77
    assert schedule(lib, class3(0, 0)).poll_waves == 77
    monkeypatch.setenv("HYPO_POA_CAPS", "5,5,5,3")
    assert schedule(lib, class3(0, 514)).poll_cap == 3


def test_rare_grid_hint(lib):
    hint = lambda h, n=N_C2, cls=3: lib.sched_rare_grid_hint(C.byref(h), cls, C.c_uint32(n))
    assert hint(history()) == 32                            # history valid, last count 0, planned 0
    assert hint(history(valid=False)) == 256
    assert hint(history(last_count=(0, 0, 0, 514), last_planned=(0, 0, 0, 0))) == 1027          # 514 + 257 + 256
    assert hint(history(valid=False), n=100) == 100
    s = schedule(lib, history(last_count=(59780, 20392, 16906, 514, 3), last_planned=(59780, 20392, 16906, 0, 1)))
    assert (s.hint3, s.hint4, s.hint5, s.mopup4) == (1027, 259, 32, 259)
    # classes below 3: the floor max(n / 8, 256)
    late = lambda h, cls, n: lib.sched_late_arrivals(C.byref(h), cls, C.c_uint32(n))
    assert late(history(), 1, N_C2) == N_C2 // 8
    assert late(history(), 2, 1000) == 256
    assert late(history(last_count=(0, 0, 100), last_planned=(0, 0, 60)), 2, N_C2) == 40 + 20 + N_C2 // 8


def test_sequential(lib, monkeypatch):
    seq = lambda last3, valid=True: bool(schedule(lib, history(valid=valid, last_count=(59780, 20392, 16906, last3))).sequential)
    assert seq(9708) and not seq(9707) and not seq(9708, valid=False)
    monkeypatch.setenv("HYPO_POA_SEQUENTIAL", "1")
    assert seq(0) and seq(0, valid=False)
    monkeypatch.setenv("HYPO_POA_SEQUENTIAL", "0")
    assert not seq(50000)


def test_class0_geometry_and_fixed_shares(lib, monkeypatch):
    s = schedule(lib, history())
    assert not s.four_groups and list(s.caps) == [5, 5, 5] and s.order == b"201"
    # ... adapt off: a measurement of the same geometry changes nothing
    assert list(schedule(lib, history(work=(9 * 10**8, 10**8, 10**8), gw=32)).caps) == [5, 5, 5]
    s = schedule(lib, history(planned=(86, 10, 4)), n=100)
    assert s.four_groups and list(s.caps) == [7, 6, 5]
    assert not schedule(lib, history(planned=(85, 10, 5)), n=100).four_groups
    monkeypatch.setenv("HYPO_POA_CLASS0", "16")
    assert schedule(lib, history()).four_groups
    monkeypatch.setenv("HYPO_POA_CLASS0", "32")
    assert not schedule(lib, history(planned=(86, 10, 4)), n=100).four_groups
    monkeypatch.delenv("HYPO_POA_CLASS0")
    monkeypatch.setenv("HYPO_POA_CAPS", "4,4,5")
    assert list(schedule(lib, history()).caps) == [4, 4, 5]
    assert list(schedule(lib, history(planned=(86, 10, 4), work=(9 * 10**8, 10**8, 10**8), gw=16), n=100).caps) == [4, 4, 5]
    monkeypatch.setenv("HYPO_POA_ADAPT", "1")
    assert list(schedule(lib, history(work=(9 * 10**8, 10**8, 10**8), gw=32)).caps) == [4, 4, 5]
    monkeypatch.delenv("HYPO_POA_CAPS")
    monkeypatch.setenv("HYPO_POA_ORDER", "021")
    assert schedule(lib, history()).order == b"021"
    monkeypatch.setenv("HYPO_POA_ORDER", "02")                 # not three characters: ignored
    assert schedule(lib, history()).order == b"201"


def brute_force_shares(work, fp, fp3, poll_waves_per_cu, caps):
    """pick_wave_shares again: the best time first, then most waves within 3 % of it"""
    lds_budget = 160.0 * 1024.0 * 1.05 - poll_waves_per_cu * float(fp3[0])
    vgpr_budget = 2048.0 - poll_waves_per_cu * float(fp3[1]) * 0.5
    fits = [(w0, w1, w2) for w0 in range(1, fp[0][2] + 1) for w1 in range(1, fp[1][2] + 1) for w2 in range(1, fp[2][2] + 1)
            if float(w0) * fp[0][0] + float(w1) * fp[1][0] + float(w2) * fp[2][0] <= lds_budget
            and float(w0) * fp[0][1] + float(w1) * fp[1][1] + float(w2) * fp[2][1] <= vgpr_budget]
    time = lambda w: max(float(work[0]) / w[0], float(work[1]) / w[1], float(work[2]) / w[2])
    best_t = min(time(w) for w in fits)
    best, best_sum = list(caps), 0
    for w in fits:
        if time(w) <= best_t * 1.03 and sum(w) > best_sum:
            best, best_sum = list(w), sum(w)
    return best


def test_wave_shares(lib, monkeypatch):
    dense = dict(planned=(86, 10, 4), gw=16)
    assert list(schedule(lib, history(work=(0, 0, 0), **dense), n=100).caps) == [7, 6, 5]                  # nothing measured
    assert list(schedule(lib, history(work=(9 * 10**8, 10**14 + 1, 10**8), **dense), n=100).caps) == [7, 6, 5]   # implausible read
    assert list(schedule(lib, history(work=(9 * 10**8, 10**8, 10**8), planned=(86, 10, 4), gw=32), n=100).caps) == [7, 6, 5]   # measured in the other geometry
    assert list(schedule(lib, history(valid=False, work=(9 * 10**8, 10**8, 10**8), **dense), n=100).caps) == [7, 6, 5]
    fp4 = (FP[0], FP[2], FP[3])
    for work, planned3, poll in (((912345678, 71234567, 13456789), 0, 0), ((500000000, 400000000, 300000000), 2, 1),
                                 ((10**9, 10**7, 10**9), 500, 2)):
        want = brute_force_shares(work, fp4, FP[4], poll, [7, 6, 5])
        got = list(schedule(lib, history(work=work, planned=(8600, 1000, 400, planned3), gw=16), n=10000 + planned3).caps)
        assert got == want and want != [7, 6, 5], (work, got, want)
    # HYPO_POA_ADAPT=1: the model on a mixed batch too (two groups per wave: the other footprint of class 0); =0: nowhere
    monkeypatch.setenv("HYPO_POA_ADAPT", "1")
    work = (300000000, 200000000, 700000000)
    assert list(schedule(lib, history(work=work, gw=32)).caps) == brute_force_shares(work, (FP[1], FP[2], FP[3]), FP[4], 0, [5, 5, 5])
    monkeypatch.setenv("HYPO_POA_ADAPT", "0")
    assert list(schedule(lib, history(work=(912345678, 71234567, 13456789), **dense), n=100).caps) == [7, 6, 5]


def test_history_builder(lib):
    def build(pin, have, waited, prev=(0,) * 8, n=100000, hw=50000):
        h = History()
        lib.sched_history(C.byref(pin), int(have), int(waited), (C.c_uint32 * 8)(*prev), C.c_uint32(n), C.c_uint32(hw), C.byref(h))
        return h
    pin = Pinned()
    pin.plan[3], pin.final_count[3] = 10, 300
    pin.work[0], pin.work[1], pin.work[2], pin.work[6] = 111, 222, 333, 16
    h = build(pin, True, False)                               # not waiting: the previous call's numbers, scaled by 100000 / 50000
    assert (h.planned[3], h.last_count[3], h.last_planned[3]) == (20, 600, 20)
    assert list(h.work) == [111, 222, 333] and h.measured_gw == 16 and h.valid
    prev = (1, 2, 3, 7, 5, 6, 0, 0)
    h = build(pin, True, True, prev)                          # waiting, with history: this call's plan, the pinned finals, the last call's plan
    assert (h.planned[3], h.last_count[3]) == (10, 300) and list(h.last_planned) == list(prev)
    assert list(h.work) == [111, 222, 333] and h.valid
    h = build(pin, False, True, prev)                         # waiting without history
    assert h.planned[3] == 10 and list(h.last_count) == [0] * 8 and list(h.last_planned) == [0] * 8
    assert list(h.work) == [0, 0, 0] and not h.valid
    pin.plan[0] = 4000000000                                  # (the scaling is done in 64 bits)
    assert build(pin, True, False, n=50000, hw=100000).planned[0] == 2000000000


@pytest.mark.parametrize("occupancy,cap,cus,gpw,clamp,group_cap,windows,grid", [
    (8, 1, 256, 1, True, 2560, 64, 64), (8, 2, 256, 1, True, 2560, 5000, 512), (10, 0, 256, 1, True, 2048, 5000, 2048),
    (8, 5, 256, 4, False, 0, 0, 1), (0, 0, 256, 1, True, 16, 0, 1),
    (8, 5, 256, 2, False, 0, 59780, 1280), (8, 5, 256, 4, False, 0, 1001, 251), (10, 0, 256, 1, True, 16, 5000, 16)])
def test_grid(lib, occupancy, cap, cus, gpw, clamp, group_cap, windows, grid):
    assert lib.sched_grid(occupancy, cap, cus, gpw, int(clamp), group_cap, C.c_uint32(windows)) == grid


def test_grid_waves_per_cu_knob(lib, monkeypatch):
    monkeypatch.setenv("HYPO_POA_WAVES_PER_CU", "3")
    assert lib.sched_grid(8, 5, 256, 1, 0, 0, C.c_uint32(100000)) == 768
    assert lib.sched_grid(8, 2, 256, 1, 0, 0, C.c_uint32(100000)) == 512


def test_remaining_decisions(lib):
    long4 = lambda p4, groups4=64: schedule(lib, history(planned=(59780, 20392, 16906, 0, p4)), groups4=groups4)
    assert long4(1).long_first_pass and long4(64).long_first_pass and long4(64).first4 == 64
    assert not long4(0).long_first_pass and not long4(65).long_first_pass
    side = lambda groups3, poll_groups: bool(lib.sched_side_by_side(groups3, C.c_uint32(poll_groups)))
    assert side(2560, 64) and side(2560, 2496) and not side(2560, 2497) and not side(2560, 0) and not side(64, 8) and side(72, 8)


# hypo_gpu_poa_workspace_bytes(n_windows, n_arms) for n_arms in N_ARMS, as the library answered before the layout got a function of its own
N_ARMS = (0, 1, 1024, 1025, 600000)
WORKSPACE_BYTES = {
    1: (254103808, 254104320, 254112256, 254112512, 258908672),
    15: (948516992, 948517504, 948525440, 948525696, 953321856),
    16: (1011645440, 1011645952, 1011653888, 1011654144, 1016450304),
    17: (1074807168, 1074807680, 1074815616, 1074815872, 1079612032),
    2559: (6904563200, 6904563712, 6904571648, 6904571904, 6909368064),
    2560: (6904597504, 6904598016, 6904605952, 6904606208, 6909402368),
    2561: (6904599296, 6904599808, 6904607744, 6904608000, 6909404160),
    97078: (7004219904, 7004220416, 7004228352, 7004228608, 7009024768),
    400000: (7323499264, 7323499776, 7323507712, 7323507968, 7328304128),
    5000000: (8125641216, 8125641728, 8125649664, 8125649920, 8130446080),
}


def test_workspace(lib):
    gpu = capi.load_library()                                 # (a pure function: no device needed)
    up = lambda b: (b + 255) // 256 * 256
    for n, want in WORKSPACE_BYTES.items():
        assert tuple(int(gpu.hypo_gpu_poa_workspace_bytes(C.c_uint32(n), C.c_uint32(a))) for a in N_ARMS) == want
        L = Layout()
        lib.sched_layout(C.c_uint32(n), C.byref(L))
        for off in (L.queues, L.keys, L.carry, L.spill, L.dirg3, L.scratch):
            assert off % 256 == 0
        assert L.queues == 8192 and L.keys == up(L.queues + 6 * 4 * n) and L.carry == L.keys + up(2 * n) and L.spill == L.carry + up(4 * n)
        assert L.spill_bytes == min(max(n * 1024, 1 << 20), 1 << 30) and L.dirg3 == L.spill + L.spill_bytes
        assert L.groups3 == min(max(n, 16), 2560) and L.scratch == L.dirg3 + L.groups3 * 33280 and L.prefix == L.scratch
        # what follows the prefix does not depend on the layout: the scratch of classes 4 / 5 and the arm offsets
        assert want[0] > L.prefix and want[1] - want[0] == 512 and want[3] - want[0] == up(1025 * 8) + 256


def test_under_sanitizers():
    """everything above once more against the harness built with -fsanitize=address,undefined"""
    if os.environ.get("HYPO_SCHED_LIB"):
        return                                                  # (this is that run)
    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "emu"), "sched"])
    libasan = subprocess.check_output(["gcc", "-print-file-name=libasan.so"], text=True).strip()
    env = dict(os.environ, LD_PRELOAD=libasan, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0", UBSAN_OPTIONS="halt_on_error=1",
               HYPO_SCHED_LIB="libhypo_sched_asan.so")
    p = subprocess.run([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", "-m", "not gpu", os.path.abspath(__file__)],
                       env=env, capture_output=True, text=True, timeout=900, cwd=os.path.dirname(HERE))
    assert p.returncode == 0 and " passed" in p.stdout and "failed" not in p.stdout, (p.stdout[-1500:], p.stderr[-1500:])
