#!/usr/bin/env python3
"""hypo --kmer-bridge on the MI355X: the rate of hypo_gpu_kset_query_walks on the sites of a real run's own intervals, and what the
flag adds to the wall time of `hypo` on BASELINE config C3 (DESIGN.md "k-mer bridge").

    python profiles/bridge_rate.py --out DIR [--parent-bin PATH]      # everything below, in one call
      1. e2e_c3_100m_s31 (100 x 1 Mbp, -p 10) is generated in a scratch directory and polished once without a flag.
      2. a child builds the 21-mer set of the run's reads, asks hypo_gpu_kset_query_track for the intervals of the polished texts
         (ten contigs a call, as the run's batches), picks the sites by the rule of the flag (max 64, slack 8) and makes the walks
         call over each batch at budget 4096: one warm-up round, then 5 timed rounds (sites/s and steps/s of the entry, upload of
         the text included, without the track calls), and the statuses it answered.
      3. `hypo` on C3, --wall-runs alternated runs each (default 5; process wall): no flag, no flag with the parent commit's binary
         (--parent-bin: hypo of a build of the parent, beside its two libraries), --kmer-bridge.
    python profiles/bridge_rate.py --sites-only polished.fasta --reads reads.fa      # (the child of step 2)
"""
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
MAX_DIST, SLACK, BUDGET = 64, 8, 4096
PIECE = 256 << 20
REPS = 5
BATCH = 10                    # contigs a call: -p of the C3 run


def pick_sites(text, off, iv_off, start, end):
    """the sites of the texts text[off[i]:off[i + 1]] by the flag's rule: (from, to, dlo, dhi) in positions of `text`"""
    is_base = np.zeros(256, bool)
    is_base[np.frombuffer(b"ACGTacgt", np.uint8)] = True
    bad = np.concatenate([[0], np.cumsum(~is_base[text])])
    frm, to, dlo, dhi = [], [], [], []
    for i in range(off.size - 1):
        s, e = (x[int(iv_off[i]):int(iv_off[i + 1])].astype(np.int64) for x in (start, end))
        if not s.size:
            continue
        length = int(off[i + 1] - off[i])
        a, b = s - 1, e - K + 1
        d0 = b - a
        ok = (a >= 0) & (b + K <= length) & (d0 >= 2) & (d0 <= MAX_DIST)
        gap = s[1:] - e[:-1]
        ok[1:] &= gap >= 2
        ok[:-1] &= gap >= 2
        a, b, d0 = a[ok] + int(off[i]), b[ok] + int(off[i]), d0[ok]
        clean = (bad[a + K] == bad[a]) & (bad[b + K] == bad[b])
        a, b, d0 = a[clean], b[clean], d0[clean]
        frm.append(a); to.append(b); dlo.append(np.maximum(1, d0 - SLACK)); dhi.append(d0 + SLACK)
    cat = lambda x, t: np.concatenate(x).astype(t) if x else np.zeros(0, t)
    return cat(frm, np.uint64), cat(to, np.uint64), cat(dlo, np.uint32), cat(dhi, np.uint32)


def sites_calls(fasta, reads):
    import edit_checker as ec
    from hypo_amd import abi, capi
    contigs = [s.encode() for _, s in ec.read_fastx(fasta)]
    gpu = capi.HypoGpu(0)
    data = np.fromfile(reads, dtype=np.uint8)
    gpu.kset_begin(K, sum(len(c) for c in contigs))
    t0 = time.perf_counter()
    for at in range(0, data.size, PIECE - (K - 1)):
        gpu.kset_add(data[at:at + PIECE])
    t_set = time.perf_counter() - t0
    del data
    batches, n_iv, t_track = [], 0, 0.0
    for b in range(0, len(contigs), BATCH):
        part = contigs[b:b + BATCH]
        text = np.frombuffer(b"".join(part), np.uint8)
        off = np.concatenate([[0], np.cumsum([len(c) for c in part])]).astype(np.uint64)
        t0 = time.perf_counter()
        _, _, iv_off, start, end, _ = gpu.kset_query_track(text.tobytes(), off)
        t_track += time.perf_counter() - t0
        n_iv += int(iv_off[-1])
        batches.append((text, pick_sites(text, off, iv_off, start, end)))
    n_sites = sum(int(s[0].size) for _, s in batches)
    out = {"contigs": len(contigs), "text_bytes": sum(len(c) for c in contigs), "intervals": n_iv, "sites": n_sites, "max": MAX_DIST, "slack": SLACK, "budget": BUDGET,
           "set_build_s": round(t_set, 3), "track_calls_s": round(t_track, 3), "distinct": gpu.kset_size()[0]}
    ts, got = [], None
    for rep in range(REPS + 1):                              # the first round is the warm-up: arenas grown, code loaded
        t0 = time.perf_counter()
        got = [gpu.kset_query_walks(text, *s, BUDGET)[:3] for text, s in batches if s[0].size]
        if rep:
            ts.append(time.perf_counter() - t0)
    status = np.concatenate([g[0] for g in got]) if got else np.zeros(0, np.uint32)
    steps = np.concatenate([g[1] for g in got]) if got else np.zeros(0, np.uint32)
    n_steps = int(steps.astype(np.int64).sum())
    out.update({"round_s": [round(t, 4) for t in ts], "best_s": round(min(ts), 4), "sites_per_s": round(n_sites / min(ts)) if n_sites else 0,
                "steps": n_steps, "steps_per_s": round(n_steps / min(ts)) if n_sites else 0, "most_steps_of_a_site": int(steps.max()) if steps.size else 0,
                "unique": int((status == abi.WALK_UNIQUE).sum()), "none": int((status == abi.WALK_NONE).sum()), "ambiguous": int((status == abi.WALK_AMBIGUOUS).sum()),
                "over_budget": int((status == abi.WALK_BUDGET).sum())})
    gpu.kset_end()
    return out


def wall(argv, cwd):
    env = dict(os.environ, HYPO_REQUIRE_DEVICE="1")
    t0 = time.perf_counter()
    p = subprocess.run(argv, cwd=cwd, env=env, capture_output=True, text=True, timeout=1200)
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
    ap.add_argument("--sites-only")
    ap.add_argument("--reads")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--wall-runs", type=int, default=5)
    ap.add_argument("--parent-bin", help="hypo of a build of the parent commit (flag-off comparison)")
    args = ap.parse_args()
    if args.sites_only:
        print(json.dumps(sites_calls(args.sites_only, args.reads)))
        return
    import e2e_util as eu
    out = os.path.abspath(args.out)
    os.makedirs(out, exist_ok=True)
    work = tempfile.mkdtemp(prefix="bridge_rate_")
    res = {"what": f"hypo --kmer-bridge, k = {K}, max {MAX_DIST}, slack {SLACK}, BASELINE config C3 (100 x 1 Mbp, 30x 150-bp reads)"}

    def save():
        json.dump(res, open(os.path.join(out, "bridge_rate.json"), "w"), indent=1)
    name = "e2e_c3_100m_s31"
    d = os.path.join(work, "set_" + name)                  # (a scratch directory: the set is GBs)
    os.makedirs(d)
    man, p, dt, _ = eu.run_fast_case(name, d, threads=args.threads)
    argv = [eu.BIN] + man["command"].split()[1:]
    if "our_p" in man["args"] and "-p" in argv:
        argv[argv.index("-p") + 1] = str(man["args"]["our_p"])
    argv[argv.index("-t") + 1] = str(args.threads)
    res["run"] = {"first_run_s": round(dt, 2)}
    reads = os.path.join(d, argv[argv.index("-r") + 1])
    child = [sys.executable, os.path.abspath(__file__), "--sites-only", os.path.join(d, "hypo_draft.fasta"), "--reads", reads]
    p = subprocess.run(["timeout", "-k", "10", "600"] + child, capture_output=True, text=True)
    if p.returncode != 0:                                  # (nothing more on the GPU after a failed child)
        print(p.stderr[-1500:], flush=True)
        shutil.rmtree(work, ignore_errors=True)
        raise SystemExit(1)
    res["entry"] = json.loads(p.stdout.strip().splitlines()[-1])
    print(json.dumps(res["entry"]), flush=True)
    save()
    # wall time on C3: alternated
    kinds = {"no_flag": (argv, []), "bridge": (argv, ["--kmer-bridge", "b.tsv"])}
    if args.parent_bin:
        kinds["no_flag_parent"] = ([os.path.abspath(args.parent_bin)] + argv[1:], [])
    runs = {k: [] for k in kinds}
    info = None
    for i in range(args.wall_runs):
        for kind, (base, extra) in kinds.items():
            dt, stdout = wall(base + extra, d)
            runs[kind].append(dt)
            if kind == "bridge":
                info = [l for l in stdout.splitlines() if "k-mer bridge" in l]
        print("wall", i, {k: round(v[-1], 3) for k, v in runs.items()}, flush=True)
        res["c3_wall"] = {k: spread(v) for k, v in runs.items()}
        save()
    res["run"]["bridge_info"] = info[0] if info else None
    res["c3_wall"]["bridge_over_no_flag_median_pct"] = round(100 * (np.median(runs["bridge"]) / np.median(runs["no_flag"]) - 1), 2)
    if args.parent_bin:
        res["c3_wall"]["no_flag_vs_parent_median_pct"] = round(100 * (np.median(runs["no_flag"]) / np.median(runs["no_flag_parent"]) - 1), 2)
    print(json.dumps(res["c3_wall"]), flush=True)
    shutil.rmtree(work, ignore_errors=True)
    save()


if __name__ == "__main__":
    main()
