"""CPU: hypo_gpu_kset_query_fixes is an additive entry point of C-ABI 11.  The header declares it with its signature and its two
limits, the library exports it, hypo_amd/capi.py lists it, without a device it answers HYPO_E_NOTINIT with its outputs untouched, and
the version is still 11 everywhere."""
import os
import re
import subprocess
import sys

import pytest

from hypo_amd import abi, capi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAME = "hypo_gpu_kset_query_fixes"


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        capi.build_library()
    return capi.load_library()


def header():
    return open(os.path.join(ROOT, "include", "hypo_gpu.h")).read()


def test_declared_with_its_signature():
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    assert re.search(r"\bint\s+" + NAME + r"\s*\(\s*const char\* bytes,\s*uint64_t n_bytes,\s*const uint64_t\* lo,\s*const uint64_t\* hi,\s*"
                     r"const uint64_t\* c0,\s*const uint64_t\* c1,\s*uint32_t n_sites,\s*uint64_t\* none_total,\s*uint64_t\* none_missing,\s*"
                     r"uint32_t\* best_cand,\s*uint64_t\* best_total,\s*uint64_t\* best_missing,\s*uint32_t\* zeros,\s*"
                     r"uint64_t\* cand_total\s*,\s*uint64_t\* cand_missing\s*\)\s*;", text)
    assert re.search(r"#define\s+HYPO_KSET_MAX_FIX_REGION\s+31\b", text) and abi.KSET_MAX_FIX_REGION == 31
    assert re.search(r"#define\s+HYPO_KSET_MAX_FIX_SPAN\s+2048\b", text) and abi.KSET_MAX_FIX_SPAN == 2048


def test_exported_and_listed(lib):
    assert hasattr(lib, NAME), f"libhypo_gpu.so does not export {NAME}"
    assert NAME in capi.EXPORTS
    assert callable(getattr(capi.HypoGpu, "kset_query_fixes")) and callable(getattr(capi.HypoGpu, "kset_query_fixes_rc"))


def test_version_is_still_11(lib):
    assert re.search(r"#define\s+HYPO_GPU_ABI_VERSION\s+(\d+)", header()).group(1) == "11"
    assert abi.ABI_VERSION == 11
    assert lib.hypo_gpu_abi_version() == 11


NOTINIT = r"""
import ctypes as C
import numpy as np
from hypo_amd import abi, capi
lib = capi.load_library()
pos = [np.array([v], np.uint64) for v in (0, 40, 18, 22)]
out64 = [np.full(1, 7, np.uint64) for _ in range(4)]
out32 = [np.full(1, 7, np.uint32) for _ in range(2)]
cand = [np.full(33, 7, np.uint64) for _ in range(2)]
p = lambda a: a.ctypes.data_as(C.c_void_p)
rc = lib.hypo_gpu_kset_query_fixes(b"ACGT" * 10, C.c_uint64(40), p(pos[0]), p(pos[1]), p(pos[2]), p(pos[3]), C.c_uint32(1), p(out64[0]), p(out64[1]), p(out32[0]),
                                   p(out64[2]), p(out64[3]), p(out32[1]), p(cand[0]), p(cand[1]))
assert rc == abi.HYPO_E_NOTINIT, rc
assert b"hypo_gpu_init" in lib.hypo_gpu_last_error()
assert all(a.tolist() == [7] * a.size for a in out64 + out32 + cand)
print("notinit ok")
"""


def test_needs_hypo_gpu_init():
    """in a process of its own: the library has not been initialised there, whether or not the machine has a device"""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-c", NOTINIT], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "notinit ok" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
