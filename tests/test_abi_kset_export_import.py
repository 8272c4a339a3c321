"""CPU: hypo_gpu_kset_export and hypo_gpu_kset_import are additive entry points of C-ABI 11.  The header declares both with their
signatures and the end-of-sequence cursor, hypo_amd/abi.py mirrors it, the library exports them, hypo_amd/capi.py lists them and
has the four methods, without a device each answers HYPO_E_NOTINIT with its outputs untouched, and the version is still 11
everywhere."""
import os
import re
import subprocess
import sys

import pytest

from hypo_amd import abi, capi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAMES = ("hypo_gpu_kset_export", "hypo_gpu_kset_import")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        capi.build_library()
    return capi.load_library()


def header():
    return open(os.path.join(ROOT, "include", "hypo_gpu.h")).read()


def test_declared_with_their_signatures():
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    assert re.search(r"\bint\s+hypo_gpu_kset_export\s*\(\s*uint64_t\* cursor,\s*uint64_t\* keys,\s*uint8_t\* counts\s*,\s*uint64_t cap,\s*uint64_t\* n_out,\s*"
                     r"uint64_t\* digest\s*\)\s*;", text)
    assert re.search(r"\bint\s+hypo_gpu_kset_import\s*\(\s*const uint64_t\* keys,\s*const uint8_t\* counts\s*,\s*uint64_t n,\s*uint64_t\* digest\s*\)\s*;", text)
    assert re.search(r"#define\s+HYPO_KSET_EXPORT_END\s+0xffffffffffffffffull\b", text)
    assert abi.KSET_EXPORT_END == 0xFFFFFFFFFFFFFFFF
    # the contract comment spells the digest out
    for word in ("0x9e3779b97f4a7c15", "0xff51afd7ed558ccd", "0xc4ceb9fe1a85ec53", "x >> 33", "Additive to ABI 11"):
        assert word in header(), word


def test_exported_and_listed(lib):
    for name in NAMES:
        assert hasattr(lib, name), f"libhypo_gpu.so does not export {name}"
        assert name in capi.EXPORTS
    for method in ("kset_export", "kset_export_rc", "kset_import", "kset_import_rc"):
        assert callable(getattr(capi.HypoGpu, method)), method


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
keys, counts = np.full(4, 7, np.uint64), np.full(4, 7, np.uint8)
cursor, n_out, digest = C.c_uint64(0), C.c_uint64(7), C.c_uint64(7)
rc = lib.hypo_gpu_kset_export(C.byref(cursor), p(keys), p(counts), C.c_uint64(4), C.byref(n_out), C.byref(digest))
assert rc == abi.HYPO_E_NOTINIT, rc
assert b"hypo_gpu_init" in lib.hypo_gpu_last_error()
assert (cursor.value, n_out.value, digest.value) == (0, 7, 7) and keys.tolist() == [7] * 4 and counts.tolist() == [7] * 4
rc = lib.hypo_gpu_kset_import(p(keys), p(counts), C.c_uint64(4), C.byref(digest))
assert rc == abi.HYPO_E_NOTINIT, rc
assert b"hypo_gpu_init" in lib.hypo_gpu_last_error()
assert digest.value == 7 and keys.tolist() == [7] * 4 and counts.tolist() == [7] * 4
print("notinit ok")
"""


def test_needs_hypo_gpu_init():
    """in a process of its own: the library has not been initialised there, whether or not the machine has a device"""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-c", NOTINIT], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "notinit ok" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
