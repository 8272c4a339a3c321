#!/usr/bin/env python3
"""hypo --qv-cn on the MI355X: hypo_gpu_kset_query_depth next to hypo_gpu_kset_query_track (the pass of --qv-bed) on the same text
and set (DESIGN.md "k-mer copy number").

    python profiles/cn_rate.py --out DIR      # writes DIR/cn_rate.json
      1. e2e_c3_100m_s31 (100 x 1 Mbp, -p 10) is generated in a scratch directory and polished once.
      2. that generator brings an empty reads.fa, so the 21-mer set is built from the polished text itself, every contig once and
         every second contig a second time (read counts 1 and 2), counting, and the text is marked into plane 0: every window is
         present and rated, which is the most work the depth kernel does per window.
      3. one warm-up call of each entry, then 5 timed calls each, alternated, in one process, through ctypes on the same arrays.
"""
import argparse
import ctypes as C
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
K = 21
BIN = 1024
REPS = 5


def spread(ts):
    ts = np.array(ts)
    return {"runs_s": [round(float(t), 4) for t in ts], "median_s": round(float(np.median(ts)), 4), "min_s": round(float(ts.min()), 4), "max_s": round(float(ts.max()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--threads", type=int, default=16)
    args = ap.parse_args()
    import e2e_util as eu
    import edit_checker as ec
    from hypo_amd import capi
    from hypo_amd.capi import _p
    out = os.path.abspath(args.out)
    os.makedirs(out, exist_ok=True)
    work = tempfile.mkdtemp(prefix="cn_rate_")
    try:
        _, _, dt, _ = eu.run_fast_case("e2e_c3_100m_s31", work, threads=args.threads)
        seqs = [s.encode() for _, s in ec.read_fastx(os.path.join(work, "hypo_draft.fasta"))]
    finally:
        shutil.rmtree(work, ignore_errors=True)
    gpu = capi.HypoGpu(0)
    gpu.kset_begin(K, sum(len(s) for s in seqs))
    gpu.kset_counts_enable(1)
    gpu.kset_add(b"\n".join(seqs))
    gpu.kset_add(b"\n".join(seqs[::2]))
    gpu.kset_mark(0, seqs)
    text = b"".join(seqs)
    n = len(seqs)
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
    data = np.frombuffer(text + b"\0", dtype=np.uint8)
    counted = gpu.kset_query_track_rc(text, off)                # warm-up and the counting call
    n_iv = int(counted[3][-1])
    n_bins = int(sum(-(-len(s) // BIN) for s in seqs))
    warm = gpu.kset_query_depth_rc(text, off, bin=BIN, text=0, unit=1)
    assert warm[0] == 0 and warm[1].size == n_bins
    tt, tm = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    iv_off, iv = np.zeros(n + 1, np.uint64), [np.zeros(n_iv + 1, np.uint64) for _ in range(3)]
    u32, med = [np.zeros(n_bins, np.uint32) for _ in range(5)], np.zeros(n_bins, np.uint8)
    t_track, t_depth = [], []
    for _ in range(REPS):
        t0 = time.perf_counter()
        rc_t = gpu.lib.hypo_gpu_kset_query_track(_p(data), _p(off), C.c_uint32(n), None, _p(tt), _p(tm), _p(iv_off), *[_p(a) for a in iv], C.c_uint64(n_iv))
        t_track.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        rc_d = gpu.lib.hypo_gpu_kset_query_depth(_p(data), _p(off), C.c_uint32(n), C.c_uint32(BIN), C.c_uint32(0), C.c_uint32(1), C.c_uint64(n_bins), *[_p(a) for a in u32], _p(med))
        t_depth.append(time.perf_counter() - t0)
        assert rc_t == 0 and rc_d == 0 and int(u32[0].sum()) == int(tt.sum()) and int(u32[1].sum()) == int(tm.sum())
    res = {"what": f"hypo_gpu_kset_query_depth (bin {BIN}) next to hypo_gpu_kset_query_track, k = {K}, the polished text of BASELINE config C3 (100 x 1 Mbp)",
           "polish_run_s": round(dt, 2), "sequences": n, "text_bytes": len(text), "distinct": gpu.kset_size()[0], "windows": int(tt.sum()), "missing": int(tm.sum()),
           "bins": n_bins, "rated": int(u32[2].sum()), "over": int(u32[3].sum()), "under": int(u32[4].sum()), "track": spread(t_track), "depth": spread(t_depth)}
    gpu.kset_end()
    json.dump(res, open(os.path.join(out, "cn_rate.json"), "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
