"""hypo --vcf on the MI355X: the rate of hypo_gpu_edit_scripts on the replacement units of real runs, and what --vcf adds to the wall
time of `hypo` on BASELINE config C3 (DESIGN.md "Edit scripts").

    python profiles/edit_rate.py --out DIR            # everything below, in one call
      1. e2e_c4s_5m_s55 (5 x 1 Mbp, -B) and e2e_c3_100m_s31 (100 x 1 Mbp, -p 10) are generated (in a scratch directory) and
         polished once with HYPO_REGION_DUMP; their units (tests/edit_checker.units_from_dump) are saved as units_<set>.npz.
      2. the entry on each set's units: one warm-up call, then 5 timed calls (units/s, bytes/s, full-matrix-equivalent cells/s).
      3. `rocprofv3 --kernel-trace --stats` around a child that makes the same calls: launches and kernel time per entry call
         (TotalDurationNs / the child's 6 calls).
      4. `hypo` on C3 with and without --vcf, alternated, --wall-runs runs each (default 3; process wall).
    python profiles/edit_rate.py --entry-only units_<set>.npz   # (the child of step 3)
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


def entry_calls(path, reps):
    from hypo_amd import capi
    z = np.load(path)
    a, b, ao, bo = z["a"].tobytes(), z["b"].tobytes(), z["a_off"], z["b_off"]
    al = [a[ao[i]:ao[i + 1]] for i in range(ao.size - 1)]
    bl = [b[bo[i]:bo[i + 1]] for i in range(bo.size - 1)]
    gpu = capi.HypoGpu(0)
    gpu.edit_scripts_raw(al, bl)                        # warm-up: scratch grown, code loaded
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        dist, off, runs = gpu.edit_scripts_raw(al, bl)
        ts.append(time.perf_counter() - t0)
    n = np.diff(ao).astype(np.float64)
    m = np.diff(bo).astype(np.float64)
    return {"units": len(al), "draft_bytes": int(ao[-1]), "text_bytes": int(bo[-1]), "identical": int(np.sum(dist == 0)),
            "edits": int(dist.sum()), "runs": int(off[-1]), "call_s": [round(t, 4) for t in ts], "best_s": round(min(ts), 4),
            "units_per_s": round(len(al) / min(ts)), "full_matrix_cells_per_s": float(np.sum(n * m)) / min(ts)}


def prepare(name, outdir, threads):
    import e2e_util as eu
    import edit_checker as ec
    d = os.path.join(outdir, "set_" + name)      # (outdir: a scratch directory — the sets are GBs)
    shutil.rmtree(d, ignore_errors=True)
    os.makedirs(d)
    man, p, dt, _ = eu.run_fast_case(name, d, threads=threads, extra_env={"HYPO_REGION_DUMP": os.path.join(d, "regions.tsv")})
    argv = [eu.BIN] + man["command"].split()[1:]
    if "our_p" in man["args"] and "-p" in argv:
        argv[argv.index("-p") + 1] = str(man["args"]["our_p"])
    argv[argv.index("-t") + 1] = str(threads)
    drafts = {n: s.upper() for n, s in ec.read_fastx(os.path.join(d, "draft.fa"))}
    names = list(drafts)
    units, _ = ec.units_from_dump(os.path.join(d, "regions.tsv"), names, drafts, "-B" in argv)
    a, b = [], []
    for n in names:
        for beg, end, t in units[n]:
            a.append(drafts[n][beg:end].encode())
            b.append(t.encode())
    ao = np.concatenate([[0], np.cumsum([len(x) for x in a])]).astype(np.uint64)
    bo = np.concatenate([[0], np.cumsum([len(x) for x in b])]).astype(np.uint64)
    path = os.path.join(outdir, f"units_{name}.npz")
    np.savez(path, a=np.frombuffer(b"".join(a), dtype=np.uint8), b=np.frombuffer(b"".join(b), dtype=np.uint8), a_off=ao, b_off=bo)
    os.remove(os.path.join(d, "regions.tsv"))
    return path, d, argv, dt


def wall(argv, cwd, vcf):
    a = list(argv) + (["--vcf", "edits.vcf"] if vcf else [])
    env = dict(os.environ, HYPO_REQUIRE_DEVICE="1")
    t0 = time.perf_counter()
    p = subprocess.run(a, cwd=cwd, env=env, capture_output=True, text=True, timeout=1200)
    dt = time.perf_counter() - t0
    if p.returncode != 0:
        raise SystemExit(f"hypo failed ({p.returncode}): {p.stderr[-1500:]}")
    info = [l for l in p.stdout.splitlines() if "Info: VCF" in l]
    return dt, info[0] if info else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--entry-only")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--wall-runs", type=int, default=3, help="runs of `hypo` on C3 with and without --vcf (alternated)")
    args = ap.parse_args()
    if args.entry_only:
        print(json.dumps(entry_calls(args.entry_only, 5)))
        return
    out = os.path.abspath(args.out)
    os.makedirs(out, exist_ok=True)
    work = tempfile.mkdtemp(prefix="edit_rate_")
    res = {}
    sets = {}
    for name in ("e2e_c4s_5m_s55", "e2e_c3_100m_s31"):
        path, d, argv, dt = prepare(name, work, args.threads)
        sets[name] = (path, d, argv)
        res[name] = {"first_run_s": round(dt, 2), "entry": entry_calls(path, 5)}
        print(name, json.dumps(res[name]), flush=True)
    # kernel time: rocprofv3 around a child that makes the same calls (its own process, the program after --)
    for name, (path, _, _) in sets.items():
        pdir = os.path.join(out, "rocprof_" + name)
        cmd = ["timeout", "-k", "10", "600", "rocprofv3", "--kernel-trace", "--stats", "-d", pdir, "-o", "edit", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--entry-only", path]
        p = subprocess.run(cmd, capture_output=True, text=True)
        import csv
        stats, per_call = [], {}
        n_calls = 1 + 5                                   # the child's warm-up call and its timed calls
        for root, _, files in os.walk(pdir):
            for f in files:
                if f.endswith("kernel_stats.csv"):
                    stats += [l for l in open(os.path.join(root, f)).read().splitlines() if "edit_" in l or l.startswith('"Name"')]
                    for row in csv.DictReader(open(os.path.join(root, f))):
                        if "edit_" in row["Name"]:
                            k = row["Name"].split("(")[0].replace("void hypo::", "")
                            per_call[k] = {"launches_per_call": int(row["Calls"]) / n_calls,
                                           "ms_per_call": round(float(row["TotalDurationNs"]) / n_calls / 1e6, 3)}
        res[name]["rocprof_rc"] = p.returncode
        res[name]["kernel_stats"] = stats
        res[name]["kernels_per_entry_call"] = per_call
        print(name, "kernel stats:", *stats, json.dumps(per_call), sep="\n", flush=True)
        if p.returncode != 0:                         # (nothing more on the GPU after a failed child)
            print(p.stderr[-1500:], flush=True)
            shutil.rmtree(work, ignore_errors=True)
            json.dump(res, open(os.path.join(out, "edit_rate.json"), "w"), indent=1)
            raise SystemExit(1)
    # --vcf on C3: alternated, --wall-runs runs each
    _, d, argv = sets["e2e_c3_100m_s31"]
    runs = {"without": [], "with": []}
    info = None
    for _ in range(args.wall_runs):
        runs["without"].append(round(wall(argv, d, False)[0], 3))
        dt, info = wall(argv, d, True)
        runs["with"].append(round(dt, 3))
    res["c3_wall"] = {"without_s": runs["without"], "with_s": runs["with"], "vcf_info": info,
                      "overhead_median_pct": round(100 * (np.median(runs["with"]) / np.median(runs["without"]) - 1), 2)}
    print(json.dumps(res["c3_wall"]), flush=True)
    shutil.rmtree(work, ignore_errors=True)
    json.dump(res, open(os.path.join(out, "edit_rate.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
