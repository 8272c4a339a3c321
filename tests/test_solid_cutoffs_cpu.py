"""CPU: the cut-offs of the solid k-mer construction against the REAL suk::SolidKmers::find_cutoffs
(tests/golden/solid_cutoffs.json.gz, made by tests/golden/make_solid_cutoffs_golden.py): the host library's C++ restatement
(hypo_host_solid_cutoffs, host/SolidBuild.cpp) and the CPU checker's (tests/solid_checker.py) give the reference's
{err, mean, lower, upper} on every case, and both report the cases where the reference's result is undefined."""
import ctypes as C
import gzip
import json
import os

import numpy as np
import pytest

import solid_checker as sc
from hypo_amd import capi

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = json.loads(gzip.open(os.path.join(HERE, "golden", "solid_cutoffs.json.gz")).read())


@pytest.fixture(scope="module")
def host():
    from hypo_amd.host import HostMirror
    if not os.path.exists(capi.LIB_PATH):
        capi.build_library()
    return HostMirror().lib


def host_cutoffs(lib, hist):
    h = np.array([x & 0xFFFFFFFFFFFFFFFF for x in hist], dtype=np.uint64)
    out = (C.c_uint32 * 4)()
    rc = lib.hypo_host_solid_cutoffs(h.ctypes.data_as(C.c_void_p), C.c_uint32(h.size), out)
    return None if rc != 0 else [out[0], out[1], out[2], out[3]]


def test_golden_covers_the_contract():
    names = [c["name"] for c in CASES]
    assert len(CASES) > 400
    assert any(n.startswith("reads_") for n in names) and any(n.startswith("planB") for n in names)
    assert any(n.startswith("errth_gt100") for n in names) and any("_x" in n for n in names)
    assert any(c["result"] == "undefined" for c in CASES)
    assert any(c["result"] != "undefined" and c["result"][3] == len(c["hist"]) - 1 for c in CASES), "no upper == 4c case"
    assert any(max(c["hist"]) >= 1 << 32 for c in CASES)


def test_host_cutoffs_equal_reference(host):
    bad = []
    for c in CASES:
        got = host_cutoffs(host, c["hist"])
        want = None if c["result"] == "undefined" else c["result"]
        if got != want:
            bad.append((c["name"], got, want))
    assert not bad, bad[:5]


def test_checker_cutoffs_equal_reference():
    bad = []
    for c in CASES:
        got = sc.find_cutoffs(c["hist"])
        want = None if c["result"] == "undefined" else tuple(c["result"])
        if got != want:
            bad.append((c["name"], got, want))
    assert not bad, bad[:5]


def test_undefined_gives_error_code(host):
    h = np.array([0, 0, 5, 3, 1, 0, 0, 0, 0], dtype=np.uint64)
    out = (C.c_uint32 * 4)()
    assert host.hypo_host_solid_cutoffs(h.ctypes.data_as(C.c_void_p), C.c_uint32(h.size), out) == -1
