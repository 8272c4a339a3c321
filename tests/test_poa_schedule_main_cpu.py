"""Which first pass rides the caller's stream (PoaSchedule::main_class, hypo_amd/csrc/poa_sched.hpp), pinned without a GPU through
tests/emu/sched_main_cases.cpp: the class with the largest wave-time per wave of its share in the last finished call, class 2
whenever that call says nothing usable; HYPO_POA_MAIN forces; the new byte sits in padding and moves no other field."""
import ctypes as C
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
N_C2 = 97078
C2 = (59780, 20392, 16906)                 # the C2 batch's windows in classes 0 - 2: two 32-lane groups per wave of class 0
KNOBS = ("CLASS0", "SEQUENTIAL", "SYNC_PLAN", "CAPS", "ORDER", "POLL", "POLL_WAVES", "ADAPT", "ADAPT_LOG", "WAVES_PER_CU", "MAIN")


class Schedule(C.Structure):
    _fields_ = [("sequential", C.c_bool), ("four_groups", C.c_bool), ("caps", C.c_int * 3), ("order", C.c_char * 4),
                ("long_first_pass", C.c_bool), ("main_class", C.c_uint8), ("first4", C.c_uint32), ("poll_waves", C.c_uint32),
                ("poll_cap", C.c_int), ("hint3", C.c_uint32), ("hint4", C.c_uint32), ("hint5", C.c_uint32), ("mopup4", C.c_uint32)]


@pytest.fixture(scope="module")
def lib():
    out = os.path.join(HERE, "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libhypo_sched_main.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-fPIC", "-shared", "-o", so,
                           os.path.join(HERE, "emu", "sched_main_cases.cpp")])
    return C.CDLL(so)


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv("HYPO_POA_" + k, raising=False)


def schedule(lib, work=(0, 0, 0), planned=C2, gw=32, valid=True, n=N_C2):
    s = Schedule()
    got = lib.sched_main((C.c_uint32 * 3)(*planned), (C.c_uint64 * 3)(*work), C.c_uint64(gw), int(valid), C.c_uint32(n), C.byref(s))
    assert got == s.main_class
    return s


def main(lib, *a, **kw):
    return schedule(lib, *a, **kw).main_class


E5 = 10**5
LONGEST0 = (1145 * E5, 741 * E5, 1097 * E5)       # wave-times of the C2 step: class 0 is the longest kernel


def test_layout(lib):
    out = (C.c_uint64 * 5)()
    lib.sched_main_layout(out)
    assert list(out) == [52, 20, 21, 24, 48]
    assert C.sizeof(Schedule) == 52 and Schedule.main_class.offset == 21
    assert Schedule.first4.offset == 24 and Schedule.mopup4.offset == 48


def test_class_2_unless_the_history_says_otherwise(lib):
    assert main(lib, LONGEST0, valid=False) == 2                       # no history
    assert main(lib, LONGEST0, gw=16) == 2                              # measured with class 0 in the other geometry
    assert main(lib, LONGEST0, planned=(86, 10, 4), gw=32, n=100) == 2  # ... either way round
    assert main(lib, (0, 0, 0)) == 2                                    # nothing measured
    assert main(lib, (1145 * E5, 10**14 + 1, 1097 * E5)) == 2           # implausible (a torn read)
    assert main(lib, (1100 * E5, 700 * E5, 1100 * E5)) == 2             # a tie with class 2
    assert main(lib, (1100 * E5, 1100 * E5, 900 * E5)) == 2             # a tie of the other two: nobody is longest


def test_longest_class(lib):
    s = schedule(lib, LONGEST0)
    assert list(s.caps) == [5, 5, 5] and s.main_class == 0 and not s.sequential and s.order == b"201"
    assert main(lib, (700 * E5, 700 * E5, 1100 * E5)) == 2
    assert main(lib, (700 * E5, 1200 * E5, 900 * E5)) == 1
    # the dense geometry, measured in it: the shares come from the same work (pick_wave_shares), class 0 stays longest with every wave that fits
    s = schedule(lib, (9000 * E5, 10 * E5, 1 * E5), planned=(86, 10, 4), gw=16, n=100)
    assert s.four_groups and list(s.caps) != [7, 6, 5] and 9000 * s.caps[1] > 10 * s.caps[0] and s.main_class == 0


def test_per_wave_of_the_share(lib, monkeypatch):
    monkeypatch.setenv("HYPO_POA_CAPS", "8,5,5")                        # 1145 / 8 < 1097 / 5
    s = schedule(lib, LONGEST0)
    assert list(s.caps) == [8, 5, 5] and s.main_class == 2
    monkeypatch.setenv("HYPO_POA_CAPS", "5,2,5")                        # 741 / 2 is the largest
    assert main(lib, LONGEST0) == 1


def test_knob_forces(lib, monkeypatch):
    for v in (0, 1, 2):
        monkeypatch.setenv("HYPO_POA_MAIN", str(v))
        assert main(lib, LONGEST0) == v and main(lib, (700 * E5, 1200 * E5, 900 * E5)) == v and main(lib, LONGEST0, valid=False) == v
    for junk in ("3", "-1", "", "01", "x"):                             # not one of 0, 1, 2: ignored
        monkeypatch.setenv("HYPO_POA_MAIN", junk)
        assert main(lib, LONGEST0) == 0 and main(lib, LONGEST0, valid=False) == 2


def test_sequential_is_unaffected(lib, monkeypatch):
    monkeypatch.setenv("HYPO_POA_SEQUENTIAL", "1")
    a, b = schedule(lib, LONGEST0), schedule(lib, (0, 0, 0))
    assert a.sequential and a.main_class == 2 and bytes(a) == bytes(b)
    monkeypatch.setenv("HYPO_POA_MAIN", "0")                            # ... the knob included
    assert bytes(schedule(lib, LONGEST0)) == bytes(a)
