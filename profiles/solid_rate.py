#!/usr/bin/env python3
"""Stage 0 on the MI355X: the solid k-mer set built from 30x short reads (profiles/gen_reads.py) through the same host code a run
of `hypo` without -i uses (hypo_host_solid_build: streaming parser, double-buffered page-locked chunks, hypo_gpu_kmer_*).
Prints one JSON line: per set the stage-0 wall time, host parse rate, bytes sent to the device, the host-side time of the count
calls with k-mers/s, and the peak device memory (hipMemGetInfo sampled every 2 ms while the stage runs).
    python profiles/solid_rate.py [--sets 5m:11,100m:13,20m:17] [--dir /tmp/solid_rate] [--kernel-trace]
--kernel-trace: every set once more, alone, under `rocprofv3 --kernel-trace --stats`; the per-kernel totals of its
kernel_stats.csv are added to the line."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import threading
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)


def parse_size(s):
    return int(float(s[:-1]) * {"k": 1e3, "m": 1e6, "g": 1e9}[s[-1].lower()]) if s[-1].isalpha() else int(s)


def reads_for(d, size):
    import gen_reads
    path = os.path.join(d, f"reads_{size}.fa")
    if not os.path.exists(path):
        gen_reads.generate(path + ".part", parse_size(size))
        os.replace(path + ".part", path)
    return path


def one(path, k, cov=30):
    import torch
    from hypo_amd import capi
    gpu = capi.HypoGpu(0)
    free0, _ = torch.cuda.mem_get_info(0)
    low = [free0]
    stop = threading.Event()

    def sample():
        while not stop.is_set():
            low[0] = min(low[0], torch.cuda.mem_get_info(0)[0])
            time.sleep(0.002)
    th = threading.Thread(target=sample)
    th.start()
    t0 = time.perf_counter()
    r = gpu.solid_kmers_build([path], k, cov)
    wall = time.perf_counter() - t0
    stop.set()
    th.join()
    parse, count, hist, fill, total = r["times"]
    n_kmers = r["seq_bytes"] - (k - 1) * (r["seq_bytes"] // 151)          # 150-bp reads, one separator each (upper bound with Ns)
    return {"k": k, "wall_s": round(wall, 3), "stage_s": round(total, 3), "parse_s": round(parse, 3),
            "parse_GBps": round(r["file_bytes"] / parse / 1e9, 3) if parse else None, "file_GB": round(r["file_bytes"] / 1e9, 3),
            "sent_to_device_GB": round(r["seq_bytes"] / 1e9, 3), "count_calls_s": round(count, 3),
            "count_kmers_per_s": round(n_kmers / count, 0) if count else None, "histogram_s": round(hist, 4), "set_s": round(fill, 3),
            "peak_device_GiB": round((free0 - low[0]) / 2 ** 30, 3), "cut": r["cut"], "n_canonical": r["n_canonical"]}


def kernel_stats(path, k, out_dir):
    d = os.path.join(out_dir, f"kt_k{k}")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "run", "--", sys.executable, os.path.abspath(__file__),
           "--one", f"{path}:{k}"]
    subprocess.run(cmd, check=True, timeout=900, capture_output=True)
    out = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            name = " ".join(str(v) for v in row.values())
            calls = next((row[c] for c in row if c.lower() == "calls"), "0")
            total = next((row[c] for c in row if c.lower().startswith("totalduration")), "0")
            for short in ("kmer_count_kernel", "kmer_histogram_kernel", "solid_fill_kernel"):
                if short in name:
                    out[short] = {"calls": int(calls), "total_ms": round(float(total) / 1e6, 3)}
    if not out:
        out["files"] = sorted(os.path.relpath(f, d) for f in glob.glob(os.path.join(d, "**", "*"), recursive=True))[:20]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="5m:11,100m:13,20m:17")
    ap.add_argument("--dir", default="/tmp/solid_rate")
    ap.add_argument("--kernel-trace", action="store_true")
    ap.add_argument("--one", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        path, k = a.one.rsplit(":", 1)
        print(json.dumps(one(path, int(k))))
        return
    os.makedirs(a.dir, exist_ok=True)
    res = {"what": "solid k-mer set from 30x 150-bp reads (stage 0)", "sets": {}}
    for spec in a.sets.split(","):
        size, k = spec.split(":")
        path = reads_for(a.dir, size)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", f"{path}:{k}"], capture_output=True, text=True,
                           timeout=1800)
        if p.returncode != 0:
            raise SystemExit(p.stderr[-2000:])
        row = json.loads(p.stdout.strip().splitlines()[-1])
        if a.kernel_trace:
            row["kernels"] = kernel_stats(path, int(k), a.dir)
        res["sets"][f"{size}_k{k}"] = row
    print(json.dumps(res))


if __name__ == "__main__":
    main()
