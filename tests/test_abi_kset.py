"""CPU: C-ABI 11.  The header, hypo_amd/abi.py and the built library agree on the version, and the library exports the five
hypo_gpu_kset_* entry points the header declares; without a device they answer HYPO_E_NOTINIT."""
import ctypes as C
import os
import re

import pytest

from hypo_amd import abi, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KSET = ["hypo_gpu_kset_begin", "hypo_gpu_kset_add", "hypo_gpu_kset_size", "hypo_gpu_kset_query", "hypo_gpu_kset_end"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        capi.build_library()
    return capi.load_library()


def header():
    return open(os.path.join(ROOT, "include", "hypo_gpu.h")).read()


def test_version_11_everywhere(lib):
    assert re.search(r"#define\s+HYPO_GPU_ABI_VERSION\s+(\d+)", header()).group(1) == "11"
    assert abi.ABI_VERSION == 11
    assert lib.hypo_gpu_abi_version() == 11


def test_kset_symbols_declared_and_exported(lib):
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name in KSET:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), f"{name} is not declared in hypo_gpu.h"
        assert hasattr(lib, name), f"libhypo_gpu.so does not export {name}"
        assert name in capi.EXPORTS
    assert re.search(r"hypo_gpu_kset_begin\s*\(\s*uint32_t k,\s*uint64_t expected_distinct,\s*uint64_t max_bytes\s*\)", text)
    assert re.search(r"hypo_gpu_kset_query\s*\(\s*const char\* bytes,\s*const uint64_t\* off,\s*uint32_t n_seqs,\s*uint64_t\* total,\s*uint64_t\* missing\s*\)", text)


def test_kset_calls_need_a_device(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    n = C.c_uint64(0)
    assert lib.hypo_gpu_kset_begin(C.c_uint32(21), C.c_uint64(1000), C.c_uint64(0)) == abi.HYPO_E_NOTINIT
    assert lib.hypo_gpu_kset_add(b"ACGT" * 10, C.c_uint64(40)) == abi.HYPO_E_NOTINIT
    assert lib.hypo_gpu_kset_size(C.byref(n), None) == abi.HYPO_E_NOTINIT
    assert b"hypo_gpu_init" in lib.hypo_gpu_last_error()
