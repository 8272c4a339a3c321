#!/usr/bin/env python3
"""hypo --kmer-bridge-vote on the MI355X: the rate of hypo_gpu_kset_query_walk_sets on 2^16 two-walk sites, and what the flag adds to
the wall time of `hypo` on BASELINE config C3 (DESIGN.md "k-mer bridge vote").

    python profiles/vote_rate.py --out DIR [--parent-bin PATH]        # everything below, in one call
      1. a child builds a counting 21-mer set from error-free 100-base reads of a random truth of 128 kb, every position about 36
         times (a 21-mer is in about 28 of them), with 2 more reads that carry another base at each of 1024 positions 120 bases apart (the `minor` sites of
         tests/test_gpu_kset_walks.py: two walks, about 30 against 2), and asks the entry for the 1024 sites 64 times over, 2^16
         sites a call at budget 4096: one warm-up round, then 5 timed rounds (sites/s and steps/s of the entry, upload of the text
         and the copies back included), next to the walks entry on the same sites.  The generated C3 set has no reads, hence no
         k-mer and no site (DESIGN.md "k-mer bridge"): no rate is taken from it.
      2. e2e_c3_100m_s31 (100 x 1 Mbp, -p 10) is generated in a scratch directory and polished once without a flag; then `hypo` on
         C3, --wall-runs alternated runs each (default 5; process wall): no flag, no flag with the parent commit's binary
         (--parent-bin: hypo of a build of the parent, beside its two libraries), --kmer-bridge, --kmer-bridge --kmer-bridge-vote 4.
    python profiles/vote_rate.py --entry-only                         # (the child of step 1)
Every step that uses the GPU is a child under a time limit of its own; after one that fails nothing more is started."""
import argparse
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
SLACK, BUDGET = 8, 4096
REPS = 5
TRUTH, SPACING, N_ALT, TIMES = 128 * 1024, 120, 1024, 64


def entry_calls():
    from hypo_amd import abi, capi
    rng = np.random.default_rng(2026)
    truth = rng.choice(np.frombuffer(b"ACGT", np.uint8), TRUTH)
    reads = [truth[i:i + 100].tobytes() for i in range(0, TRUTH - 99, 3)] + [truth[i:i + 100].tobytes() for i in range(1, TRUTH - 99, 30)]
    pos = 1000 + SPACING * np.arange(N_ALT)
    for p in pos:
        r = truth[p - 50:p + 50].copy()
        r[50] = b"ACGT"[(b"ACGT".index(bytes([r[50]])) + 1) % 4]
        reads += [r.tobytes()] * 2
    blob = b"\n".join(reads)
    gpu = capi.HypoGpu(0)
    gpu.kset_begin(K, TRUTH)
    gpu.kset_counts_enable(1)
    gpu.kset_add(blob)
    a, b = pos - 2 - K, pos + 3
    tile = lambda x, t: np.tile(x, TIMES).astype(t)
    sites = (tile(a, np.uint64), tile(b, np.uint64), tile(np.maximum(1, b - a - SLACK), np.uint32), tile(b - a + SLACK, np.uint32))
    n_sites = sites[0].size
    out = {"k": K, "truth_bytes": TRUTH, "reads": len(reads), "distinct": gpu.kset_size()[0], "sites": n_sites, "distinct_sites": N_ALT, "budget": BUDGET}
    text = truth.tobytes()
    for name, call in (("walk_sets", gpu.kset_query_walk_sets), ("walks", gpu.kset_query_walks)):
        ts, got = [], None
        for rep in range(REPS + 1):                          # the first round is the warm-up: arenas grown, code loaded
            t0 = time.perf_counter()
            got = call(text, *sites, BUDGET)
            if rep:
                ts.append(time.perf_counter() - t0)
        status, steps = got[0], got[1]
        n_steps = int(steps.astype(np.int64).sum())
        out[name] = {"round_s": [round(t, 4) for t in ts], "best_s": round(min(ts), 4), "sites_per_s": round(n_sites / min(ts)), "steps": n_steps,
                     "steps_per_s": round(n_steps / min(ts)), "most_steps_of_a_site": int(steps.max()),
                     "status": {str(v): int((status == v).sum()) for v in np.unique(status)}}
        if name == "walk_sets":
            nw, low = got[2], got[4]
            two = nw == 2
            out[name].update({"two_walks": int(two.sum()), "median_best_support": int(np.median(low[two][:, :2].max(axis=1))) if two.any() else 0,
                              "median_second_support": int(np.median(low[two][:, :2].min(axis=1))) if two.any() else 0})
    gpu.kset_end()
    return out


def wall(argv, cwd):
    env = dict(os.environ, HYPO_REQUIRE_DEVICE="1")
    t0 = time.perf_counter()
    p = subprocess.run(["timeout", "-k", "10", "300"] + argv, cwd=cwd, env=env, capture_output=True, text=True)
    dt = time.perf_counter() - t0
    if p.returncode != 0:
        raise SystemExit(f"hypo failed ({p.returncode}): {p.stderr[-1500:]}")
    return dt, p.stdout


def spread(ts):
    ts = np.array(ts)
    return {"runs_s": [round(float(t), 3) for t in ts], "median_s": round(float(np.median(ts)), 3), "min_s": round(float(ts.min()), 3),
            "max_s": round(float(ts.max()), 3), "std_s": round(float(ts.std(ddof=1)), 3) if ts.size > 1 else 0.0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--entry-only", action="store_true")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--wall-runs", type=int, default=5)
    ap.add_argument("--parent-bin", help="hypo of a build of the parent commit (flag-off comparison)")
    args = ap.parse_args()
    if args.entry_only:
        print(json.dumps(entry_calls()))
        return
    import e2e_util as eu
    out = os.path.abspath(args.out)
    os.makedirs(out, exist_ok=True)
    res = {"what": f"hypo --kmer-bridge-vote 4, k = {K}; the entry on 2^16 generated two-walk sites; the flags on BASELINE config C3 (100 x 1 Mbp, its reads file is empty)"}

    def save():
        json.dump(res, open(os.path.join(out, "vote_rate.json"), "w"), indent=1)
    p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--entry-only"], capture_output=True, text=True)
    if p.returncode != 0:                                  # (nothing more on the GPU after a failed child)
        print(p.stdout[-1500:], p.stderr[-1500:], flush=True)
        raise SystemExit(1)
    res["entry"] = json.loads(p.stdout.strip().splitlines()[-1])
    print(json.dumps(res["entry"]), flush=True)
    save()
    work = tempfile.mkdtemp(prefix="vote_rate_")
    name = "e2e_c3_100m_s31"
    d = os.path.join(work, "set_" + name)                  # (a scratch directory: the set is GBs)
    os.makedirs(d)
    man, p, dt, _ = eu.run_fast_case(name, d, threads=args.threads)
    argv = [eu.BIN] + man["command"].split()[1:]
    if "our_p" in man["args"] and "-p" in argv:
        argv[argv.index("-p") + 1] = str(man["args"]["our_p"])
    argv[argv.index("-t") + 1] = str(args.threads)
    res["run"] = {"first_run_s": round(dt, 2)}
    kinds = {"no_flag": (argv, []), "bridge": (argv, ["--kmer-bridge", "b.tsv"]), "bridge_vote": (argv, ["--kmer-bridge", "v.tsv", "--kmer-bridge-vote", "4"])}
    if args.parent_bin:
        kinds["no_flag_parent"] = ([os.path.abspath(args.parent_bin)] + argv[1:], [])
    runs = {k: [] for k in kinds}
    info = None
    for i in range(args.wall_runs):
        for kind, (base, extra) in kinds.items():
            dt, stdout = wall(base + extra, d)
            runs[kind].append(dt)
            if kind == "bridge_vote":
                info = [l for l in stdout.splitlines() if "k-mer bridge" in l]
        print("wall", i, {k: round(v[-1], 3) for k, v in runs.items()}, flush=True)
        res["c3_wall"] = {k: spread(v) for k, v in runs.items()}
        save()
    res["run"]["bridge_info"] = info
    med = lambda k: float(np.median(runs[k]))
    res["c3_wall"]["bridge_over_no_flag_median_pct"] = round(100 * (med("bridge") / med("no_flag") - 1), 2)
    res["c3_wall"]["vote_over_bridge_median_pct"] = round(100 * (med("bridge_vote") / med("bridge") - 1), 2)
    if args.parent_bin:
        res["c3_wall"]["no_flag_vs_parent_median_pct"] = round(100 * (med("no_flag") / med("no_flag_parent") - 1), 2)
    print(json.dumps(res["c3_wall"]), flush=True)
    shutil.rmtree(work, ignore_errors=True)
    save()


if __name__ == "__main__":
    main()
