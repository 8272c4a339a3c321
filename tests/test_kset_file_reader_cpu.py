"""CPU: the reader and the writer of hypo_amd/csrc/host/KmerSetFile.cpp in a small program of its own
(tests/kset_file_reader_main.cpp), built with -fsanitize=address,undefined and run as it is: no device, no code loaded into Python,
nothing preloaded.  A good file of the checker (tests/kset_file_checker.py) is accepted with its n_keys and digest, whatever the
staging buffer; every file the checker corrupts is refused with the cause named; the writer's file is the checker's, byte for byte,
and parses strictly; and the sanitisers report nothing."""
import os
import subprocess

import pytest

import kset_file_checker as kf
from test_kset_file_checker_cpu import blocks_of, reads

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BUILD = os.path.join(HERE, "_build")
PROG = os.path.join(BUILD, "kset_file_reader_main")
SRCS = [os.path.join(HERE, "kset_file_reader_main.cpp"), os.path.join(ROOT, "hypo_amd", "csrc", "host", "KmerSetFile.cpp")]
NAMED = {"bad magic": "bad magic", "bad version": "bad version", "short read": "short read", "non-zero padding": "non-zero padding",
         "would pass n_keys": "would pass n_keys", "below n_keys": "below n_keys", "bytes after the digest": "bytes after the digest"}


@pytest.fixture(scope="module")
def prog():
    os.makedirs(BUILD, exist_ok=True)
    hdr = os.path.join(ROOT, "hypo_amd", "csrc", "host", "KmerSetFile.hpp")
    if not os.path.exists(PROG) or os.path.getmtime(PROG) < max(os.path.getmtime(p) for p in SRCS + [hdr]):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-static-libasan", "-static-libubsan", "-Wall", "-Wextra", "-o", PROG] + SRCS)
    return PROG


def run(prog, *args):
    p = subprocess.run([prog] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
    return p


@pytest.fixture(scope="module")
def good():
    m = kf.model(reads(9), 21)
    return m, blocks_of(m, [5, 11, 640])


def fields(line):
    assert line.startswith("ok "), line
    return dict(f.split("=") for f in line.split()[1:])


@pytest.mark.parametrize("staging", [None, 1, 7, 640, 100000])
def test_good_file(prog, good, staging, tmp_path):
    m, blocks = good
    path = str(tmp_path / "good.hks")
    kf.write_file(path, 21, blocks)
    p = run(prog, "read", path, *([] if staging is None else [staging]))
    assert p.returncode == 0, p.stdout + p.stderr
    f = fields(p.stdout.strip())
    want = "%016x" % kf.digest(m)
    assert (f["k"], int(f["n_keys"]), int(f["records"]), f["digest"], f["sum"]) == ("21", len(m), len(m), want, want)
    # a block larger than the staging buffer is fed in pieces
    s = staging or (1 << 24)
    assert int(f["largest"]) == min(s, max(len(b) for b in blocks))
    assert int(f["pieces"]) == sum(-(-len(b) // s) for b in blocks)


def test_empty_set(prog, tmp_path):
    path = str(tmp_path / "empty.hks")
    kf.write_file(path, 31, [])
    f = fields(run(prog, "read", path).stdout.strip())
    assert (f["k"], f["n_keys"], f["records"], f["digest"]) == ("31", "0", "0", "0" * 16)


def test_corrupted_files(prog, good, tmp_path):
    m, blocks = good
    bad = kf.corrupted(21, blocks)
    assert {kf.cause_of(n) for n in bad} == set(NAMED)
    for name, data in bad.items():
        path = str(tmp_path / (name.replace(" ", "_") + ".hks"))
        open(path, "wb").write(data)
        for staging in (None, 3):
            p = run(prog, "read", path, *([] if staging is None else [staging]))
            assert p.returncode == 3, (name, p.stdout, p.stderr)
            assert p.stdout.startswith("refused: " + path + ": ") and NAMED[kf.cause_of(name)] in p.stdout, (name, p.stdout)
    p = run(prog, "read", str(tmp_path / "none.hks"))
    assert p.returncode == 3 and "none.hks" in p.stdout and "cannot be opened" in p.stdout


def test_header_alone(prog, good, tmp_path):
    """what `hypo --qv-load` reads before it sizes the table: n_keys must fit the file (9 bytes a record, a block, the end)"""
    m, blocks = good
    path = str(tmp_path / "h.hks")
    kf.write_file(path, 21, blocks)
    assert fields(run(prog, "header", path).stdout.strip()) == {"k": "21", "n_keys": str(len(m))}
    kf.write_file(path, 31, [])
    assert fields(run(prog, "header", path).stdout.strip()) == {"k": "31", "n_keys": "0"}
    one = [[(5, 1)]]
    kf.write_file(path, 21, one)                                         # the smallest file with a record: 24 + 8 + 8 + 8 + 16 bytes
    assert fields(run(prog, "header", path).stdout.strip())["n_keys"] == "1"
    for n_keys in (3, 10 ** 9, (1 << 64) - 1):
        kf.write_file(path, 21, one, n_keys=n_keys)
        p = run(prog, "header", path)
        assert p.returncode == 3 and p.stdout.startswith("refused: " + path + ": short read") and str(n_keys) in p.stdout, p.stdout
    for name in ("bad magic", "bad version", "short read in the header"):
        open(path, "wb").write(kf.corrupted(21, blocks)[name])
        p = run(prog, "header", path)
        assert p.returncode == 3 and NAMED[kf.cause_of(name)] in p.stdout, (name, p.stdout)


@pytest.mark.parametrize("cap", [1, 7, 100000])
def test_writer(prog, good, cap, tmp_path):
    m, blocks = good
    src, out = str(tmp_path / "src.hks"), str(tmp_path / "out.hks")
    kf.write_file(src, 21, blocks)
    p = run(prog, "copy", src, out, cap)
    assert p.returncode == 0, p.stdout + p.stderr
    k, n_keys, got, dig = kf.parse_file(out)
    recs = [r for b in blocks for r in b]
    assert (k, n_keys, dig) == (21, len(m), kf.digest(m)) and [r for b in got for r in b] == recs
    # one block per call that returned records: a call looks at `cap` slots, every other one of which holds a record
    at, want = 0, []
    while at < 2 * len(recs):
        want.append(recs[(at + 1) // 2:(min(at + cap, 2 * len(recs)) + 1) // 2])
        at += cap
    assert got == [b for b in want if b]
    assert fields(p.stdout.strip())["bytes"] == str(os.path.getsize(out)) and not os.path.exists(out + ".tmp")
    assert open(out, "rb").read() == kf.file_bytes(21, got)
    # a directory that does not exist: refused, nothing left
    p = run(prog, "copy", src, str(tmp_path / "no_dir" / "out.hks"), cap)
    assert p.returncode == 3 and "cannot be opened" in p.stdout
