#!/usr/bin/env python3
"""hypo --qv-bed on the MI355X: hypo_gpu_kset_query_track next to hypo_gpu_kset_query on the same text and set, and what the
flag adds to the wall time of `hypo` on BASELINE config C3 (DESIGN.md "k-mer QV track").

    python profiles/track_rate.py --out DIR      # everything below, in one call; writes DIR/track_rate.json
      1. e2e_c3_100m_s31 (100 x 1 Mbp, -p 10) is generated in a scratch directory and polished once.  (That generator brings the
         solid set in aux/ and an EMPTY reads.fa: the k-mer set of steps 2 to 4 is then empty and every window missing, which
         compares the entries' passes but is no realistic miss pattern; "distinct" in the output says which it was.)
      2. a child builds the 21-mer set of the run's reads and asks it about the polished contigs (one sequence each, one call for
         all of them): one warm-up call of each entry, then 5 timed calls each, alternated, in one process.  The track call is
         made with room for the intervals the warm-up counted, so it is one call, not the binding's two.
      3. `rocprofv3 --kernel-trace --stats` around the same child: every kset kernel's own time per call.
      4. `hypo` on C3, --wall-runs alternated runs each (default 5; process wall): --qv, --qv --qv-bed.
    python profiles/track_rate.py --entry-only hypo_draft.fasta --reads reads.fa      # (the child of steps 2 and 3)
"""
import argparse
import csv
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
K = 21
PIECE = 256 << 20
REPS = 5


def spread(ts):
    ts = np.array(ts)
    return {"runs_s": [round(float(t), 4) for t in ts], "median_s": round(float(np.median(ts)), 4), "min_s": round(float(ts.min()), 4),
            "max_s": round(float(ts.max()), 4), "std_s": round(float(ts.std(ddof=1)), 4) if ts.size > 1 else 0.0}


def entry_calls(fasta, reads):
    import edit_checker as ec
    from hypo_amd import capi
    seqs = [s.encode() for _, s in ec.read_fastx(fasta)]
    gpu = capi.HypoGpu(0)
    data = np.fromfile(reads, dtype=np.uint8)
    gpu.kset_begin(K, sum(len(s) for s in seqs))
    for at in range(0, data.size, PIECE - (K - 1)):
        gpu.kset_add(data[at:at + PIECE])
    del data
    text = b"".join(seqs)
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
    # both entries through ctypes on the same arrays: the binding's own copies of the text are not what is compared
    import ctypes as C
    from hypo_amd.capi import _p
    n = len(seqs)
    data = np.frombuffer(text + b"\0", dtype=np.uint8)
    total, missing = gpu.kset_query(seqs)                       # warm-up: arenas grown, code loaded
    counted = gpu.kset_query_track_rc(text, off)                # the counting call
    n_iv = int(counted[3][-1])
    qt, qm, tt, tm = (np.zeros(n, np.uint64) for _ in range(4))
    iv_off, iv_start, iv_end, iv_cnt = np.zeros(n + 1, np.uint64), np.zeros(n_iv + 1, np.uint64), np.zeros(n_iv + 1, np.uint64), np.zeros(n_iv + 1, np.uint64)
    t_query, t_track = [], []
    for _ in range(REPS):
        t0 = time.perf_counter()
        rc_q = gpu.lib.hypo_gpu_kset_query(_p(data), _p(off), C.c_uint32(n), _p(qt), _p(qm))
        t_query.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        rc_t = gpu.lib.hypo_gpu_kset_query_track(_p(data), _p(off), C.c_uint32(n), None, _p(tt), _p(tm), _p(iv_off), _p(iv_start), _p(iv_end), _p(iv_cnt), C.c_uint64(n_iv))
        t_track.append(time.perf_counter() - t0)
        assert rc_q == 0 and rc_t == 0 and (tt == qt).all() and (tm == qm).all() and (qt == total).all() and (qm == missing).all() and int(iv_off[-1]) == n_iv
    distinct = gpu.kset_size()[0]
    gpu.kset_end()
    return {"sequences": len(seqs), "text_bytes": len(text), "distinct": distinct, "windows": int(total.sum()), "missing": int(missing.sum()), "intervals": n_iv,
            "covered_bases": int((iv_end[:n_iv] - iv_start[:n_iv]).sum()), "query": spread(t_query), "track": spread(t_track),
            "track_over_query_median_pct": round(100 * (np.median(t_track) / np.median(t_query) - 1), 2)}


def wall(argv, cwd):
    env = dict(os.environ, HYPO_REQUIRE_DEVICE="1")
    t0 = time.perf_counter()
    p = subprocess.run(argv, cwd=cwd, env=env, capture_output=True, text=True, timeout=1200)
    dt = time.perf_counter() - t0
    if p.returncode != 0:
        raise SystemExit(f"hypo failed ({p.returncode}): {p.stderr[-1500:]}")
    return dt, p.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--entry-only")
    ap.add_argument("--reads")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--wall-runs", type=int, default=5)
    args = ap.parse_args()
    if args.entry_only:
        print(json.dumps(entry_calls(args.entry_only, args.reads)))
        return
    import e2e_util as eu
    out = os.path.abspath(args.out)
    os.makedirs(out, exist_ok=True)
    work = tempfile.mkdtemp(prefix="track_rate_")              # (a scratch directory: the set is GBs)
    res = {"what": f"hypo --qv-bed, k = {K}, BASELINE config C3 (100 x 1 Mbp, 30x 150-bp reads)"}

    def save():
        json.dump(res, open(os.path.join(out, "track_rate.json"), "w"), indent=1)

    def leave(code):
        shutil.rmtree(work, ignore_errors=True)
        raise SystemExit(code)
    name = "e2e_c3_100m_s31"
    man, p, dt, _ = eu.run_fast_case(name, work, threads=args.threads)
    argv = [eu.BIN] + man["command"].split()[1:]
    if "our_p" in man["args"] and "-p" in argv:
        argv[argv.index("-p") + 1] = str(man["args"]["our_p"])
    argv[argv.index("-t") + 1] = str(args.threads)
    res["first_run_s"] = round(dt, 2)
    child = [sys.executable, os.path.abspath(__file__), "--entry-only", os.path.join(work, "hypo_draft.fasta"), "--reads", os.path.join(work, argv[argv.index("-r") + 1])]
    p = subprocess.run(["timeout", "-k", "10", "600"] + child, capture_output=True, text=True)
    if p.returncode != 0:                                      # (nothing more on the GPU after a failed child)
        print(p.stderr[-1500:], flush=True)
        leave(1)
    res["entry"] = json.loads(p.stdout.strip().splitlines()[-1])
    print(json.dumps(res["entry"]), flush=True)
    save()
    pdir = os.path.join(out, "rocprof_track")
    p = subprocess.run(["timeout", "-k", "10", "600", "rocprofv3", "--kernel-trace", "--stats", "-d", pdir, "-o", "track", "--output-format", "csv", "--"] + child,
                       capture_output=True, text=True)
    per_call = {}
    for root, _, files in os.walk(pdir):
        for f in files:
            if f.endswith("kernel_stats.csv"):
                for row in csv.DictReader(open(os.path.join(root, f))):
                    if "kset_" in row["Name"]:
                        calls = int(row["Calls"])
                        per_call[row["Name"].split("(")[0].replace("void hypo::", "")] = {
                            "calls": calls, "ms_per_call": round(float(row["TotalDurationNs"]) / calls / 1e6, 4)}
    res["rocprof_rc"] = p.returncode
    res["kernels"] = per_call
    print(json.dumps(per_call), flush=True)
    save()
    if p.returncode != 0:
        print(p.stderr[-1500:], flush=True)
        leave(1)
    kinds = {"qv": ["--qv", "t.tsv"], "qv_bed": ["--qv", "t.tsv", "--qv-bed", "t.bed"]}
    runs = {k: [] for k in kinds}
    for i in range(args.wall_runs):
        for kind, extra in kinds.items():
            runs[kind].append(wall(argv + extra, work)[0])
        print("wall", i, {k: round(v[-1], 3) for k, v in runs.items()}, flush=True)
    res["c3_wall"] = {k: spread(v) for k, v in runs.items()}
    res["c3_wall"]["bed_over_qv_median_pct"] = round(100 * (np.median(runs["qv_bed"]) / np.median(runs["qv"]) - 1), 2)
    print(json.dumps(res["c3_wall"]), flush=True)
    save()
    leave(0)


if __name__ == "__main__":
    main()
