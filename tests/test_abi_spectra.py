"""CPU: hypo_gpu_kset_counts_enable, hypo_gpu_kset_mark and hypo_gpu_kset_spectrum are additive entry points of C-ABI 11.  The
header declares them with their signatures, the library exports them, hypo_amd/capi.py lists them, without a device they answer
HYPO_E_NOTINIT, and the version is still 11 everywhere."""
import os
import re
import subprocess
import sys

import pytest

from hypo_amd import abi, capi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAMES = ["hypo_gpu_kset_counts_enable", "hypo_gpu_kset_mark", "hypo_gpu_kset_spectrum"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        capi.build_library()
    return capi.load_library()


def header():
    return open(os.path.join(ROOT, "include", "hypo_gpu.h")).read()


def test_declared_with_their_signatures():
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    assert re.search(r"\bint\s+hypo_gpu_kset_counts_enable\s*\(\s*uint32_t n_texts\s*\)\s*;", text)
    assert re.search(r"\bint\s+hypo_gpu_kset_mark\s*\(\s*uint32_t text,\s*const char\* bytes,\s*const uint64_t\* off,\s*uint32_t n_seqs,\s*"
                     r"uint64_t\* n_windows,\s*uint64_t\* n_unmarked\s*\)\s*;", text)
    assert re.search(r"\bint\s+hypo_gpu_kset_spectrum\s*\(\s*uint32_t text,\s*uint64_t\* hist\s*\)\s*;", text)
    assert re.search(r"#define\s+HYPO_KSET_MAX_TEXTS\s+4\b", text) and abi.KSET_MAX_TEXTS == 4
    assert re.search(r"#define\s+HYPO_KSET_SPECTRUM_BINS\s+1280\b", text) and abi.KSET_SPECTRUM_BINS == 1280 == abi.KSET_SPECTRUM_ROWS * abi.KSET_SPECTRUM_COLS


def test_exported_and_listed(lib):
    for name in NAMES:
        assert hasattr(lib, name), f"libhypo_gpu.so does not export {name}"
        assert name in capi.EXPORTS
    for method in ("kset_counts_enable", "kset_counts_enable_rc", "kset_mark", "kset_mark_rc", "kset_spectrum", "kset_spectrum_rc"):
        assert callable(getattr(capi.HypoGpu, method))


def test_version_is_still_11(lib):
    assert re.search(r"#define\s+HYPO_GPU_ABI_VERSION\s+(\d+)", header()).group(1) == "11"
    assert abi.ABI_VERSION == 11
    assert lib.hypo_gpu_abi_version() == 11


NOTINIT = r"""
import ctypes as C
import numpy as np
from hypo_amd import abi, capi
lib = capi.load_library()
off, out, hist = np.array([0, 40], np.uint64), np.full(2, 7, np.uint64), np.full(abi.KSET_SPECTRUM_BINS, 7, np.uint64)
p = lambda a: a.ctypes.data_as(C.c_void_p)
for rc in (lib.hypo_gpu_kset_counts_enable(C.c_uint32(2)),
           lib.hypo_gpu_kset_mark(C.c_uint32(0), b"ACGT" * 10, p(off), C.c_uint32(1), p(out), p(out[1:])),
           lib.hypo_gpu_kset_spectrum(C.c_uint32(0), p(hist))):
    assert rc == abi.HYPO_E_NOTINIT, rc
    assert b"hypo_gpu_init" in lib.hypo_gpu_last_error()
assert out.tolist() == [7, 7] and (hist == 7).all()
print("notinit ok")
"""


def test_need_hypo_gpu_init():
    """in a process of its own: the library has not been initialised there, whether or not the machine has a device"""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-c", NOTINIT], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "notinit ok" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
