#!/usr/bin/env python3
"""The k-mer set of `hypo --qv` on the MI355X: 30x short reads (profiles/gen_reads.py) inserted through hypo_gpu_kset_add in
256 MiB calls (the file's bytes as they are: header lines end runs like any other non-base byte), then the first bytes of the
file queried as one sequence.  Writes profiles/qv_rate.json and prints it: per set the k-mers/s inside the add calls, the
growths and the time they took (HYPO_KSET_STATS line of the library), the query rate in bases/s, the final table size and load.
    python profiles/qv_rate.py [--sets 5m,100m] [--k 21] [--dir /tmp/qv_rate] [--kernel-trace] [--poly] [--counts] [--min-count]
--kernel-trace: every set once more, alone, under `rocprofv3 --kernel-trace --stats`; the kernels' own totals are added.
--poly: 150 MB of poly-A and of one read repeated, against 150 MB of the 5m set (what same-slot contention costs).
--counts: the set of `hypo --qv-spectra`.  Every set is inserted twice in one process, without counts and then with
hypo_gpu_kset_counts_enable(2) (same bytes, same calls), the queried bytes are also marked as text 0 (hypo_gpu_kset_mark) and the
spectrum is fetched (hypo_gpu_kset_spectrum); writes profiles/spectra_rate.json instead.
--min-count: the queries of `hypo --qv-min-count`.  Every set is inserted once into a set that counts (hypo_gpu_kset_counts_enable(1)), and
in the same process, on the same bytes, hypo_gpu_kset_query, hypo_gpu_kset_query_track and hypo_gpu_kset_query_spans (a million 60-byte
spans of the queried bytes, the size of the guard's) are timed at t = 1 (the presence kernels), t = 2 and t = the valley of the read
histogram (the kset_*_min_kernel variants); with --kernel-trace the kernels' own times.  Writes profiles/min_count_rate.json instead."""
import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
PIECE = 256 << 20


def parse_size(s):
    return int(float(s[:-1]) * {"k": 1e3, "m": 1e6, "g": 1e9}[s[-1].lower()]) if s[-1].isalpha() else int(s)


def reads_for(d, size):
    import gen_reads
    path = os.path.join(d, f"reads_{size}.fa")
    if not os.path.exists(path):
        gen_reads.generate(path + ".part", parse_size(size))
        os.replace(path + ".part", path)
    return path


def insert_all(gpu, data, k):
    """(seconds inside the add calls, windows handed over)"""
    t_add, at, windows = 0.0, 0, 0
    while True:
        piece = data[at:at + PIECE]
        t0 = time.perf_counter()
        gpu.kset_add(piece)
        t_add += time.perf_counter() - t0
        windows += max(0, piece.size - k + 1)
        if at + PIECE >= data.size:
            return t_add, windows
        at += PIECE - (k - 1)


def one(path, k, expected, counts=False):
    from hypo_amd import capi
    gpu = capi.HypoGpu(0)
    data = np.fromfile(path, dtype=np.uint8)
    gpu.kset_begin(k, expected)
    t_add, windows = insert_all(gpu, data, k)
    n, table_bytes = gpu.kset_size()
    q = bytes(data[:min(data.size, 64 << 20)])
    gpu.kset_query([q[:1 << 20]])                                          # (first use of the query kernel)
    t0 = time.perf_counter()
    total, missing = gpu.kset_query([q])
    t_q = time.perf_counter() - t0
    gpu.kset_end()
    row = {"k": k, "file_GB": round(data.size / 1e9, 3), "add_calls_s": round(t_add, 4), "windows": windows,
           "insert_kmers_per_s": round(windows / t_add), "distinct": n, "table_GiB": round(table_bytes / 2 ** 30, 3),
           "load": round(n * 8 / table_bytes, 3), "query_bytes": len(q), "query_s": round(t_q, 4), "query_bases_per_s": round(len(q) / t_q),
           "query_total": int(total[0]), "query_missing": int(missing[0])}
    if counts:
        # the same bytes in the same calls into a set that counts; then a mark of the queried bytes and the spectrum
        gpu.kset_begin(k, expected)
        gpu.kset_counts_enable(2)
        t_cadd, _ = insert_all(gpu, data, k)
        nc, bytes_c = gpu.kset_size()
        assert nc == n
        t0 = time.perf_counter()
        n_win, n_un = gpu.kset_mark(0, [q])
        t_m = time.perf_counter() - t0
        assert (n_win, n_un) == (int(total[0]), int(missing[0]))
        gpu.kset_spectrum(0)                                               # (first use of the kernel)
        t0 = time.perf_counter()
        hist = gpu.kset_spectrum(0)
        t_s = time.perf_counter() - t0
        assert int(hist.sum()) == n
        gpu.kset_end()
        row.update({"counts_add_calls_s": round(t_cadd, 4), "counts_insert_kmers_per_s": round(windows / t_cadd),
                    "counts_over_plain": round(t_cadd / t_add, 3), "counts_resident_GiB": round(bytes_c / 2 ** 30, 3),
                    "mark_s": round(t_m, 4), "mark_bases_per_s": round(len(q) / t_m), "spectrum_call_s": round(t_s, 5),
                    "saturated_kmers": int(hist[255].sum())})
    return row


def min_count(path, k, expected):
    """the presence kernels and the counted ones on one set, the same bytes, one process"""
    from hypo_amd import capi
    gpu = capi.HypoGpu(0)
    data = np.fromfile(path, dtype=np.uint8)
    gpu.kset_begin(k, expected)
    gpu.kset_counts_enable(1)
    insert_all(gpu, data, k)
    n, table_bytes = gpu.kset_size()
    h = gpu.kset_spectrum(0).sum(axis=1)
    valley = next((c for c in range(2, 255) if h[c] <= h[c + 1]), 2)
    q = bytes(data[:min(data.size, 64 << 20)])
    rng = np.random.default_rng(1)
    lo = rng.integers(0, len(q) - 60, 1_000_000).astype(np.uint64)
    hi = lo + np.uint64(60)
    calls = {"query": lambda: gpu.kset_query([q])[1].sum(), "track": lambda: gpu.kset_query_track([q])[1].sum(),
             "spans": lambda: gpu.kset_query_spans(q, lo, hi)[1].sum()}
    row = {"k": k, "file_GB": round(data.size / 1e9, 3), "distinct": n, "resident_GiB": round(table_bytes / 2 ** 30, 3), "valley": int(valley),
           "reliable_at_2": int(h[2:].sum()), "reliable_at_valley": int(h[valley:].sum()), "query_bytes": len(q), "spans": int(lo.size), "t": {}}
    for t in (1, 2, int(valley)):
        gpu.kset_min_count(t)
        r = {}
        for name, call in calls.items():
            call()                                                         # (first use of the kernel, arenas grown)
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                missing = int(call())
                ts.append(time.perf_counter() - t0)
            r[name] = {"call_s": [round(x, 4) for x in ts], "best_s": round(min(ts), 4), "missing": missing}
        row["t"][str(t)] = r
    gpu.kset_end()
    for t in row["t"]:
        for name in calls:
            row["t"][t][name]["over_presence"] = round(row["t"][t][name]["best_s"] / row["t"]["1"][name]["best_s"], 3)
    return row


def poly(path, k):
    from hypo_amd import capi
    gpu = capi.HypoGpu(0)
    n = 150 << 20
    rng = np.random.default_rng(1)
    read = rng.choice(list(b"ACGT"), 150).astype(np.uint8)
    sets = {"reads": np.fromfile(path, dtype=np.uint8, count=n), "poly_a": np.full(n, ord("A"), dtype=np.uint8),
            "one_read": np.tile(np.concatenate([read, [10]]).astype(np.uint8), n // 151)}
    out = {}
    for name, data in sets.items():
        gpu.kset_begin(k, 1000)
        gpu.kset_add(data[:1 << 20])                                        # (warm: code objects, arenas)
        gpu.kset_end()
        gpu.kset_begin(k, data.size)                                        # sized up front: no growth inside the timed call
        t0 = time.perf_counter()
        gpu.kset_add(data)
        dt = time.perf_counter() - t0
        out[name] = {"bytes": int(data.size), "add_s": round(dt, 4), "kmers_per_s": round(data.size / dt), "distinct": gpu.kset_size()[0]}
        gpu.kset_end()
    return out


def kernel_stats(args, out_dir, tag):
    d = os.path.join(out_dir, f"kt_{tag}")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "run", "--", sys.executable, os.path.abspath(__file__)] + args
    subprocess.run(cmd, check=True, timeout=900, capture_output=True)
    out = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            name = " ".join(str(v) for v in row.values())
            calls = next((row[c] for c in row if c.lower() == "calls"), "0")
            total = next((row[c] for c in row if c.lower().startswith("totalduration")), "0")
            for short in ("kset_insert_kernel", "kset_rehash_kernel", "kset_query_kernel", "kset_insert_count_kernel", "kset_rehash_count_kernel",
                          "kset_mark_kernel", "kset_spectrum_kernel", "kset_query_min_kernel", "kset_track_flags_kernel", "kset_track_flags_min_kernel",
                          "kset_spans_kernel", "kset_spans_min_kernel"):
                if short in name:
                    out[short] = {"calls": int(calls), "total_ms": round(float(total) / 1e6, 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="5m,100m")
    ap.add_argument("--k", type=int, default=21)
    ap.add_argument("--dir", default="/tmp/qv_rate")
    ap.add_argument("--kernel-trace", action="store_true")
    ap.add_argument("--poly", action="store_true")
    ap.add_argument("--counts", action="store_true")
    ap.add_argument("--min-count", action="store_true")
    ap.add_argument("--out")
    ap.add_argument("--one", help=argparse.SUPPRESS)
    ap.add_argument("--poly-one", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        path, size = a.one.rsplit(":", 1)
        print(json.dumps(min_count(path, a.k, int(size)) if a.min_count else one(path, a.k, int(size), a.counts)))
        return
    if a.poly_one:
        print(json.dumps(poly(a.poly_one, a.k)))
        return
    os.makedirs(a.dir, exist_ok=True)
    a.out = a.out or os.path.join(HERE, "min_count_rate.json" if a.min_count else "spectra_rate.json" if a.counts else "qv_rate.json")
    env = dict(os.environ, HYPO_KSET_STATS="1")
    res = {"what": f"exact {a.k}-mer set from 30x 150-bp reads (hypo --qv" + ("-min-count: the queries at t = 1, 2 and the valley)" if a.min_count else
                                                                               "-spectra: without and with counts)" if a.counts else ")"), "sets": {}}

    def child(args):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--k", str(a.k)] + args, capture_output=True, text=True, timeout=1800, env=env)
        if p.returncode != 0:
            raise SystemExit(p.stderr[-2000:])
        return json.loads(p.stdout.strip().splitlines()[-1]), p.stderr
    for size in a.sets.split(","):
        path = reads_for(a.dir, size)
        args = ["--one", f"{path}:{parse_size(size)}"] + (["--counts"] if a.counts else []) + (["--min-count"] if a.min_count else [])
        row, err = child(args)
        m = re.findall(r"\[kset\] k \d+, \d+ keys, \d+ slots \(peak (\d+)\), (\d+) growths in ([0-9.]+) s", err)
        if m:                                            # (--counts: the first line is the set without counts, the second the one with)
            row["peak_table_GiB"], row["growths"], row["growth_s"] = round(int(m[0][0]) * 8 / 2 ** 30, 3), int(m[0][1]), float(m[0][2])
            if a.counts and len(m) > 1:
                row["counts_growths"], row["counts_growth_s"] = int(m[1][1]), float(m[1][2])
        if a.kernel_trace:
            row["kernels"] = kernel_stats(["--k", str(a.k)] + args, a.dir, size)
        res["sets"][size] = row
    if a.poly:
        res["contention"], _ = child(["--poly-one", reads_for(a.dir, a.sets.split(",")[0])])
    text = json.dumps(res, indent=1)
    open(a.out, "w").write(text + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
