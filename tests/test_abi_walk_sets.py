"""CPU: hypo_gpu_kset_query_walk_sets is an additive entry point of C-ABI 11.  The header declares it with its signature and its two
defines, hypo_amd/abi.py mirrors them, the library exports it, hypo_amd/capi.py lists it, without a device it answers HYPO_E_NOTINIT
with its outputs untouched, and the version is still 11 everywhere."""
import os
import re
import subprocess
import sys

import pytest

from hypo_amd import abi, capi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAME = "hypo_gpu_kset_query_walk_sets"
DEFINES = [("HYPO_KSET_MAX_WALKS", 4, "KSET_MAX_WALKS"), ("HYPO_WALK_MANY", 5, "WALK_MANY")]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        capi.build_library()
    return capi.load_library()


def header():
    return open(os.path.join(ROOT, "include", "hypo_gpu.h")).read()


def test_declared_with_its_signature():
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    assert re.search(r"\bint\s+" + NAME + r"\s*\(\s*const char\* bytes,\s*uint64_t n_bytes,\s*const uint64_t\* from,\s*const uint64_t\* to,\s*"
                     r"const uint32_t\* dlo,\s*const uint32_t\* dhi,\s*uint32_t n_sites,\s*uint32_t budget,\s*uint32_t\* status,\s*uint32_t\* steps,\s*"
                     r"uint32_t\* n_walks,\s*uint32_t\* len\s*,\s*uint32_t\* low\s*,\s*uint8_t\* walk\s*\)\s*;", text)
    for name, value, mirror in DEFINES:
        assert re.search(r"#define\s+" + name + r"\s+" + str(value) + r"\b", text), name
        assert getattr(abi, mirror) == value, mirror
    # the status values of the walks entry are what they were, and MANY is none of them
    assert (abi.WALK_NONE, abi.WALK_UNIQUE, abi.WALK_AMBIGUOUS, abi.WALK_BUDGET, abi.WALK_NOANCHOR) == (0, 1, 2, 3, 4)
    # the search is written out in the header
    comment = header()[:header().index("#define HYPO_KSET_MAX_WALKS")]
    for words in ("if len(walks) == W: stop with MANY", "min(lo, c)", "visit(L, 0, \"\", 255)", "hypo_gpu_kset_counts_enable"):
        assert words in comment, words


def test_exported_and_listed(lib):
    assert hasattr(lib, NAME), f"libhypo_gpu.so does not export {NAME}"
    assert NAME in capi.EXPORTS
    assert callable(getattr(capi.HypoGpu, "kset_query_walk_sets")) and callable(getattr(capi.HypoGpu, "kset_query_walk_sets_rc"))


def test_version_is_still_11(lib):
    assert re.search(r"#define\s+HYPO_GPU_ABI_VERSION\s+(\d+)", header()).group(1) == "11"
    assert abi.ABI_VERSION == 11
    assert lib.hypo_gpu_abi_version() == 11


NOTINIT = r"""
import ctypes as C
import numpy as np
from hypo_amd import abi, capi
lib = capi.load_library()
pos = [np.array([v], np.uint64) for v in (0, 5)]
d = [np.array([v], np.uint32) for v in (1, 8)]
out32 = [np.full(n, 7, np.uint32) for n in (1, 1, 1, abi.KSET_MAX_WALKS, abi.KSET_MAX_WALKS)]
walk = np.full(abi.KSET_MAX_WALKS * abi.KSET_MAX_WALK, 7, np.uint8)
p = lambda a: a.ctypes.data_as(C.c_void_p)
rc = lib.hypo_gpu_kset_query_walk_sets(b"ACGT" * 10, C.c_uint64(40), p(pos[0]), p(pos[1]), p(d[0]), p(d[1]), C.c_uint32(1), C.c_uint32(100), p(out32[0]), p(out32[1]),
                                       p(out32[2]), p(out32[3]), p(out32[4]), p(walk))
assert rc == abi.HYPO_E_NOTINIT, rc
assert b"hypo_gpu_init" in lib.hypo_gpu_last_error()
assert all(a.tolist() == [7] * a.size for a in out32 + [walk])
print("notinit ok")
"""


def test_needs_hypo_gpu_init():
    """in a process of its own: the library has not been initialised there, whether or not the machine has a device"""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-c", NOTINIT], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "notinit ok" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
