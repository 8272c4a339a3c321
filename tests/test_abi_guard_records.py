"""CPU: hypo_gpu_kset_query_variants is an additive entry point of C-ABI 11.  The header declares it with its signature, the library
exports it, hypo_amd/capi.py lists it, without a device it answers HYPO_E_NOTINIT, and the version is still 11 everywhere."""
import os
import re
import subprocess
import sys

import pytest

from hypo_amd import abi, capi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAME = "hypo_gpu_kset_query_variants"


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        capi.build_library()
    return capi.load_library()


def header():
    return open(os.path.join(ROOT, "include", "hypo_gpu.h")).read()


def test_declared_with_its_signature():
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    args = ["const char* bytes", "uint64_t n_bytes", "const char* alts", "uint64_t n_alt_bytes", "const uint64_t* lo", "const uint64_t* hi",
            "const uint32_t* edit_off", "uint32_t n_sites", "const uint64_t* eb", "const uint64_t* ee", "const uint64_t* ao", "const uint32_t* al",
            "uint32_t* best_mask", "uint64_t* best_total", "uint64_t* best_missing", "uint64_t* var_total", "uint64_t* var_missing"]
    assert re.search(r"\bint\s+" + NAME + r"\s*\(\s*" + r"\s*,\s*".join(re.escape(a) for a in args) + r"\s*\)\s*;", text)
    assert re.search(r"#define\s+HYPO_KSET_MAX_EDITS\s+12\b", header()) and capi.KSET_MAX_EDITS == 12


def test_exported_and_listed(lib):
    assert hasattr(lib, NAME), f"libhypo_gpu.so does not export {NAME}"
    assert NAME in capi.EXPORTS
    assert callable(getattr(capi.HypoGpu, "kset_query_variants")) and callable(getattr(capi.HypoGpu, "kset_query_variants_rc"))


def test_version_is_still_11(lib):
    assert re.search(r"#define\s+HYPO_GPU_ABI_VERSION\s+(\d+)", header()).group(1) == "11"
    assert abi.ABI_VERSION == 11
    assert lib.hypo_gpu_abi_version() == 11


NOTINIT = r"""
import ctypes as C
import numpy as np
from hypo_amd import abi, capi
lib = capi.load_library()
p = lambda a: a.ctypes.data_as(C.c_void_p)
lo, hi, eoff = np.zeros(1, np.uint64), np.full(1, 30, np.uint64), np.array([0, 1], np.uint32)
eb, ee, ao, al = np.full(1, 10, np.uint64), np.full(1, 11, np.uint64), np.zeros(1, np.uint64), np.ones(1, np.uint32)
mask, out = np.zeros(1, np.uint32), np.zeros(2, np.uint64)
rc = lib.hypo_gpu_kset_query_variants(b"ACGT" * 10, C.c_uint64(40), b"T", C.c_uint64(1), p(lo), p(hi), p(eoff), C.c_uint32(1), p(eb), p(ee), p(ao), p(al),
                                      p(mask), p(out), p(out[1:]), None, None)
assert rc == abi.HYPO_E_NOTINIT, rc
assert b"hypo_gpu_init" in lib.hypo_gpu_last_error()
print("notinit ok")
"""


def test_needs_hypo_gpu_init():
    """in a process of its own: the library has not been initialised there, whether or not the machine has a device"""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-c", NOTINIT], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "notinit ok" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
