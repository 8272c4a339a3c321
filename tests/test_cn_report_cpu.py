"""CPU: host/CnReport.cpp and ReadKmerSet::query_depth / peak as a stand-alone program under AddressSanitizer and UBSan
(tests/host_cn/cn_report_main.cpp: host stand-ins for the device entry points, found by dlsym through -rdynamic).  The program
checks that a text cut into calls at contig ends, and a long contig cut at multiples of the bin with k - 1 bytes of overlap, give
the arrays of a single call; that the text is marked once and whole before the first depth call, or not at all next to a flag that
marks it; the file, its order of contigs and the sums of the Info line; the peak, and a histogram without one."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(ROOT, "hypo_amd", "csrc", "host")
OUT = os.path.join(HERE, "_build", "host_cn")


def build():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "cn_report")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-rdynamic", "-Wall", "-Wextra",
                    "-o", exe, os.path.join(HERE, "host_cn", "cn_report_main.cpp"), os.path.join(HOST, "ReadKmerSet.cpp"), os.path.join(HOST, "CnReport.cpp"), "-ldl"], check=True)
    return exe


def test_cn_report_under_sanitizers():
    p = subprocess.run([build()], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert p.stdout.strip() == "cn_report: ok" and "runtime error" not in p.stderr
