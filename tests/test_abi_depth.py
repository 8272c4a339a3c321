"""CPU: hypo_gpu_kset_query_depth is an additive entry point of C-ABI 11.  The header declares it with its signature and the two
limits of `bin`, the library exports it, hypo_amd/capi.py lists it, without a device it answers HYPO_E_NOTINIT with its arrays
untouched, and the version is still 11 everywhere."""
import os
import re
import subprocess
import sys

import pytest

from hypo_amd import abi, capi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAME = "hypo_gpu_kset_query_depth"


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        capi.build_library()
    return capi.load_library()


def header():
    return open(os.path.join(ROOT, "include", "hypo_gpu.h")).read()


def test_declared_with_its_signature():
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    assert re.search(r"\bint\s+" + NAME + r"\s*\(\s*const char\* bytes,\s*const uint64_t\* off,\s*uint32_t n_seqs,\s*uint32_t bin,\s*uint32_t text,\s*"
                     r"uint32_t unit,\s*uint64_t n_bins,\s*uint32_t\* windows,\s*uint32_t\* missing,\s*uint32_t\* rated,\s*uint32_t\* over,\s*"
                     r"uint32_t\* under,\s*uint8_t\* med_count\s*\)\s*;", text)
    assert re.search(r"#define\s+HYPO_KSET_DEPTH_MIN_BIN\s+32\b", text) and re.search(r"#define\s+HYPO_KSET_DEPTH_MAX_BIN\s+65536\b", text)
    assert (abi.KSET_DEPTH_MIN_BIN, abi.KSET_DEPTH_MAX_BIN) == (32, 65536)


def test_documented_in_the_header():
    doc = header()
    at = doc.index("int " + NAME)
    comment = doc[doc.rindex("/*", 0, at):at]
    for word in ("--qv-cn", "Additive to ABI 11", "med_count", "HYPO_E_INVALID", "n_seqs == 0 touches nothing", "Synchronous"):
        assert word in comment, word


def test_exported_and_listed(lib):
    assert hasattr(lib, NAME), f"libhypo_gpu.so does not export {NAME}"
    assert NAME in capi.EXPORTS
    assert callable(getattr(capi.HypoGpu, "kset_query_depth")) and callable(getattr(capi.HypoGpu, "kset_query_depth_rc"))


def test_version_is_still_11(lib):
    assert re.search(r"#define\s+HYPO_GPU_ABI_VERSION\s+(\d+)", header()).group(1) == "11"
    assert abi.ABI_VERSION == 11
    assert lib.hypo_gpu_abi_version() == 11


NOTINIT = r"""
import ctypes as C
import numpy as np
from hypo_amd import abi, capi
lib = capi.load_library()
off = np.array([0, 40], np.uint64)
u32 = [np.full(2, 7, np.uint32) for _ in range(5)]
med = np.full(2, 7, np.uint8)
p = lambda a: a.ctypes.data_as(C.c_void_p)
rc = lib.hypo_gpu_kset_query_depth(b"ACGT" * 10, p(off), C.c_uint32(1), C.c_uint32(32), C.c_uint32(0), C.c_uint32(1), C.c_uint64(2), *[p(a) for a in u32], p(med))
assert rc == abi.HYPO_E_NOTINIT, rc
assert b"hypo_gpu_init" in lib.hypo_gpu_last_error()
assert all(a.tolist() == [7, 7] for a in u32) and med.tolist() == [7, 7]
print("notinit ok")
"""


def test_needs_hypo_gpu_init():
    """in a process of its own: the library has not been initialised there, whether or not the machine has a device"""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-c", NOTINIT], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "notinit ok" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
