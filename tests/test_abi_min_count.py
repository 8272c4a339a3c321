"""CPU: hypo_gpu_kset_min_count is an additive entry point of C-ABI 11.  The header declares it with its signature, the library
exports it, hypo_amd/capi.py lists and wraps it, without a device it answers HYPO_E_NOTINIT, and the version is still 11 everywhere."""
import os
import re
import subprocess
import sys

import pytest

from hypo_amd import abi, capi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAME = "hypo_gpu_kset_min_count"


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        capi.build_library()
    return capi.load_library()


def header():
    return open(os.path.join(ROOT, "include", "hypo_gpu.h")).read()


def test_declared_with_its_signature():
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    assert re.search(r"\bint\s+hypo_gpu_kset_min_count\s*\(\s*uint32_t t\s*\)\s*;", text)
    doc = header()[:header().index("int hypo_gpu_kset_min_count")]
    doc = doc[doc.rindex("/*"):]
    for word in ("--qv-min-count", "Additive to ABI 11", "_query_spans", "_query_variants", "_query_track", "1..255", "HYPO_E_INVALID"):
        assert word in doc, word


def test_exported_and_mirrored(lib):
    assert hasattr(lib, NAME), f"libhypo_gpu.so does not export {NAME}"
    assert NAME in capi.EXPORTS
    for method in ("kset_min_count", "kset_min_count_rc"):
        assert callable(getattr(capi.HypoGpu, method))


def test_version_is_still_11(lib):
    assert re.search(r"#define\s+HYPO_GPU_ABI_VERSION\s+(\d+)", header()).group(1) == "11"
    assert abi.ABI_VERSION == 11
    assert lib.hypo_gpu_abi_version() == 11


NOTINIT = r"""
import ctypes as C
from hypo_amd import abi, capi
lib = capi.load_library()
for t in (0, 1, 2, 255, 256):
    assert lib.hypo_gpu_kset_min_count(C.c_uint32(t)) == abi.HYPO_E_NOTINIT
    assert b"hypo_gpu_init" in lib.hypo_gpu_last_error()
print("notinit ok")
"""


def test_needs_hypo_gpu_init():
    """in a process of its own: the library has not been initialised there, whether or not the machine has a device"""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-c", NOTINIT], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "notinit ok" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
