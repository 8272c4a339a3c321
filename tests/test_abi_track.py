"""CPU: hypo_gpu_kset_query_track is an additive entry point of C-ABI 11.  The header declares it with its signature, the library
exports it, hypo_amd/capi.py lists it, without a device it answers HYPO_E_NOTINIT, and the version is still 11 everywhere."""
import os
import re
import subprocess
import sys

import pytest

from hypo_amd import abi, capi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAME = "hypo_gpu_kset_query_track"


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        capi.build_library()
    return capi.load_library()


def header():
    return open(os.path.join(ROOT, "include", "hypo_gpu.h")).read()


def test_declared_with_its_signature():
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    assert re.search(r"\bint\s+" + NAME + r"\s*\(\s*const char\* bytes,\s*const uint64_t\* off,\s*uint32_t n_seqs,\s*const uint8_t\* want\s*,\s*"
                     r"uint64_t\* total,\s*uint64_t\* missing,\s*uint64_t\* iv_off\s*,\s*uint64_t\* iv_start,\s*uint64_t\* iv_end,\s*"
                     r"uint64_t\* iv_missing,\s*uint64_t iv_cap\s*\)\s*;", text)


def test_exported_and_listed(lib):
    assert hasattr(lib, NAME), f"libhypo_gpu.so does not export {NAME}"
    assert NAME in capi.EXPORTS
    assert callable(getattr(capi.HypoGpu, "kset_query_track")) and callable(getattr(capi.HypoGpu, "kset_query_track_rc"))


def test_version_is_still_11(lib):
    assert re.search(r"#define\s+HYPO_GPU_ABI_VERSION\s+(\d+)", header()).group(1) == "11"
    assert abi.ABI_VERSION == 11
    assert lib.hypo_gpu_abi_version() == 11


NOTINIT = r"""
import ctypes as C
import numpy as np
from hypo_amd import abi, capi
lib = capi.load_library()
off, out, iv_off = np.array([0, 40], np.uint64), np.zeros(2, np.uint64), np.full(2, 7, np.uint64)
p = lambda a: a.ctypes.data_as(C.c_void_p)
rc = lib.hypo_gpu_kset_query_track(b"ACGT" * 10, p(off), C.c_uint32(1), None, p(out), p(out[1:]), p(iv_off), None, None, None, C.c_uint64(0))
assert rc == abi.HYPO_E_NOTINIT, rc
assert b"hypo_gpu_init" in lib.hypo_gpu_last_error()
assert iv_off.tolist() == [7, 7]
print("notinit ok")
"""


def test_needs_hypo_gpu_init():
    """in a process of its own: the library has not been initialised there, whether or not the machine has a device"""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-c", NOTINIT], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "notinit ok" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
