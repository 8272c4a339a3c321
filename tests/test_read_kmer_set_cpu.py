"""CPU: host/ReadKmerSet.cpp and host/QvReport.cpp as a stand-alone program under AddressSanitizer and UBSan
(tests/host_set/read_kmer_set_main.cpp: host stand-ins for the device entry points, found by dlsym through -rdynamic).  The program
checks the set's lifecycle, the least count and its valley, and the track query's second call; a second build without one of the
set's names checks that bind() notices."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(ROOT, "hypo_amd", "csrc", "host")
OUT = os.path.join(HERE, "_build", "host_set")


def build(name, defines=()):
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, name)
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-rdynamic", "-Wall", "-Wextra",
                    *defines, "-o", exe, os.path.join(HERE, "host_set", "read_kmer_set_main.cpp"), os.path.join(HOST, "ReadKmerSet.cpp"),
                    os.path.join(HOST, "QvReport.cpp"), "-ldl"], check=True)
    return exe


@pytest.mark.parametrize("name,defines", [("read_kmer_set", ()), ("read_kmer_set_hidden", ("-DHIDE_ONE_NAME",))])
def test_read_kmer_set_under_sanitizers(name, defines):
    p = subprocess.run([build(name, defines)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert p.stdout.strip() == "read_kmer_set: ok" and "runtime error" not in p.stderr
