#!/usr/bin/env python3
"""hypo --kmer-guard and --guard-records on the MI355X: the rates of hypo_gpu_kset_query_spans and hypo_gpu_kset_query_variants on the
spans and the sites of a real run's records, and what the guard adds to the wall time of `hypo` on BASELINE config C3 (DESIGN.md "k-mer guard").

    python profiles/guard_rate.py --out DIR [--parent-bin PATH]      # everything below, in one call
      1. e2e_c3_100m_s31 (100 x 1 Mbp, -p 10) is generated in a scratch directory and polished once without a flag and once with
         --kmer-guard --vcf --qv; the clusters of the VCF's records (tests/guard_checker.clusters) give the two spans per cluster
         the host sends, over the drafts and the unguarded texts back to back.  They are saved as spans_c3.npz.
      2. a child builds the 21-mer set of the run's reads and makes the spans call with a half-wave and with a wave per span
         (HYPO_KSET_SPAN_GROUP): one warm-up call, then 5 timed calls each (spans/s of the entry, upload of the text included).
      3. `rocprofv3 --kernel-trace --stats` around the same child: the kernel's own time per call, per geometry.
      2b. the same child makes the variants call of --guard-records (hypo_gpu_kset_query_variants: one site per cluster of up to 8
         records, the records its edits, over the drafts alone) with both geometries, timed the same way; the cluster-size histogram
         and the number of clusters the call accepts in part are recorded with it.
      4. `hypo` on C3, --wall-runs alternated runs each (default 10; process wall): no flag, no flag with the parent commit's binary
         (--parent-bin: hypo of a build of the parent, beside its two libraries), --qv, --qv --kmer-guard,
         --kmer-guard, --guard-records.
    python profiles/guard_rate.py --spans-only spans_c3.npz --reads reads.fa      # (the child of steps 2 and 3)
    --min-count (either form): the child's set counts, and after the calls above (t = 1: the presence kernels) it makes them again at
    t = 2 and at the valley of the read histogram (hypo --qv-min-count: kset_spans_min_kernel, kset_variants_min_kernel), in the same
    process on the same spans and sites; the rocprofv3 pass of step 3 then lists the counted kernels next to the presence ones.
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
N_MAX = 8                     # --guard-records-max's default


def spans_calls(path, reads, min_count=False):
    from hypo_amd import capi
    z = np.load(path)
    text, lo, hi = z["text"], z["lo"], z["hi"]
    gpu = capi.HypoGpu(0)
    data = np.fromfile(reads, dtype=np.uint8)
    gpu.kset_begin(K, int(z["genome"]))
    if min_count:
        gpu.kset_counts_enable(1)                           # (t stays 1 for the first round: the presence kernels, on the same set)
    t0 = time.perf_counter()
    for at in range(0, data.size, PIECE - (K - 1)):
        gpu.kset_add(data[at:at + PIECE])
    t_set = time.perf_counter() - t0
    del data
    windows = int(np.maximum(hi.astype(np.int64) - lo.astype(np.int64) - K + 1, 0).sum())
    out = {"spans": int(lo.size), "text_bytes": int(text.size), "windows": windows, "span_bytes_mean": round(float((hi - lo).mean()), 1),
           "set_build_s": round(t_set, 3), "distinct": gpu.kset_size()[0], "groups": {}}

    def measure(out):
        """both calls, both geometries, against the set as it answers now"""
        answers = []
        for group in (32, 64):
            os.environ["HYPO_KSET_SPAN_GROUP"] = str(group)
            gpu.kset_query_spans(text, lo, hi)                  # warm-up: arenas grown, code loaded
            ts = []
            for _ in range(REPS):
                t0 = time.perf_counter()
                total, missing = gpu.kset_query_spans(text, lo, hi)
                ts.append(time.perf_counter() - t0)
            answers.append((total, missing))
            out["groups"][str(group)] = {"call_s": [round(t, 4) for t in ts], "best_s": round(min(ts), 4), "spans_per_s": round(lo.size / min(ts)),
                                         "windows_per_s": round(windows / min(ts))}
        assert all(np.array_equal(a, b) for a, b in zip(*answers)), "the two geometries disagree"
        out["missing_windows"] = int(answers[0][1].sum())
        if "v_lo" in z:                                          # the sites of --guard-records over the drafts alone
            args = (z["v_text"], z["v_alts"], z["v_lo"], z["v_hi"], z["v_eoff"], z["v_eb"], z["v_ee"], z["v_ao"], z["v_al"])
            n_edits = np.diff(z["v_eoff"].astype(np.int64))
            v = {"sites": int(z["v_lo"].size), "edits": int(n_edits.sum()), "variants": int((1 << n_edits).sum()), "text_bytes": int(z["v_text"].size),
                 "alt_bytes": int(z["v_alts"].size), "cluster_sizes": json.loads(str(z["v_hist"])), "groups": {}}
            masks = []
            for group in (32, 64):
                os.environ["HYPO_KSET_SPAN_GROUP"] = str(group)
                gpu.kset_query_variants(*args, variants=False)
                ts = []
                for _ in range(REPS):
                    t0 = time.perf_counter()
                    best = gpu.kset_query_variants(*args, variants=False)
                    ts.append(time.perf_counter() - t0)
                masks.append(best[0])
                v["groups"][str(group)] = {"call_s": [round(t, 4) for t in ts], "best_s": round(min(ts), 4), "variants_per_s": round(v["variants"] / min(ts))}
            assert np.array_equal(*masks), "the two geometries disagree"
            full = (1 << n_edits) - 1
            whole = z["v_whole"].astype(bool)                    # sites of clusters beyond the limit: one edit, decided whole
            v["rejected_whole"] = int((masks[0] == 0).sum())
            v["accepted_in_part"] = int(((masks[0] != 0) & (masks[0] != full) & ~whole).sum())
            out["variants"] = v

    measure(out)
    if min_count:                                            # --min-count: the same calls once more at t = 2 and at the valley, the kset_*_min_kernel variants
        h = gpu.kset_spectrum(0).sum(axis=1)
        valley = next((c for c in range(2, 255) if h[c] <= h[c + 1]), 2)
        out["min_count"] = {"valley": int(valley)}
        for t in (2, int(valley)):
            gpu.kset_min_count(t)
            out["min_count"][str(t)] = {"groups": {}}
            measure(out["min_count"][str(t)])
    gpu.kset_end()
    return out


def prepare(outdir, threads):
    import e2e_util as eu
    import edit_checker as ec
    import guard_checker as gc
    name = "e2e_c3_100m_s31"
    d = os.path.join(outdir, "set_" + name)                # (outdir: a scratch directory — the set is GBs)
    shutil.rmtree(d, ignore_errors=True)
    os.makedirs(d)
    man, p, dt, _ = eu.run_fast_case(name, d, threads=threads)
    argv = [eu.BIN] + man["command"].split()[1:]
    if "our_p" in man["args"] and "-p" in argv:
        argv[argv.index("-p") + 1] = str(man["args"]["our_p"])
    argv[argv.index("-t") + 1] = str(threads)
    drafts = [(n, s.upper()) for n, s in ec.read_fastx(os.path.join(d, "draft.fa"))]
    polished = dict(ec.read_fastx(os.path.join(d, "hypo_draft.fasta")))
    dt_g, out = wall(argv + ["--kmer-guard", "--vcf", "g.vcf", "--qv", "g.tsv"], d)
    info = [l for l in out.splitlines() if "k-mer guard" in l]
    _, recs = ec.parse_vcf(open(os.path.join(d, "g.vcf")).read())
    parts, lo, hi, at = [], [], [], 0
    for n, D in drafts:
        P = polished[n]
        for _, _, b, e, qb, qe in gc.clusters(recs.get(n, []), K):
            lo += [at + max(0, b - K + 1), at + len(D) + max(0, qb - K + 1)]
            hi += [at + min(len(D), e + K - 1), at + len(D) + min(len(P), qe + K - 1)]
        parts += [D, P]
        at += len(D) + len(P)
    # the sites of --guard-records: one per cluster, its records the edits (a cluster of more than N_MAX records: its polished span)
    v_lo, v_hi, v_eoff, v_eb, v_ee, v_ao, v_al, v_whole, alts, hist, at = [], [], [0], [], [], [], [], [], bytearray(), {}, 0
    for n, D in drafts:
        P, rs = polished[n], recs.get(n, [])
        for i0, i1, b, e, qb, qe in gc.clusters(rs, K):
            size = i1 - i0
            hist[str(size) if size <= N_MAX else "more"] = hist.get(str(size) if size <= N_MAX else "more", 0) + 1
            v_lo.append(at + max(0, b - K + 1)); v_hi.append(at + min(len(D), e + K - 1)); v_whole.append(size > N_MAX)
            edits = [(pos - 1, pos - 1 + len(ref), alt) for pos, ref, alt, _ in rs[i0:i1]] if size <= N_MAX else [(b, e, P[qb:qe])]
            for eb_, ee_, alt in edits:
                v_eb.append(at + eb_); v_ee.append(at + ee_); v_ao.append(len(alts)); v_al.append(len(alt)); alts += alt.encode()
            v_eoff.append(len(v_eb))
        at += len(D)
    path = os.path.join(outdir, "spans_c3.npz")
    u64 = lambda x: np.array(x, np.uint64)
    np.savez(path, text=np.frombuffer("".join(parts).encode(), dtype=np.uint8), lo=np.array(lo, np.uint64), hi=np.array(hi, np.uint64),
             genome=sum(len(D) for _, D in drafts), v_text=np.frombuffer("".join(D for _, D in drafts).encode(), dtype=np.uint8),
             v_alts=np.frombuffer(bytes(alts), dtype=np.uint8), v_lo=u64(v_lo), v_hi=u64(v_hi), v_eoff=np.array(v_eoff, np.uint32), v_eb=u64(v_eb),
             v_ee=u64(v_ee), v_ao=u64(v_ao), v_al=np.array(v_al, np.uint32), v_whole=np.array(v_whole, np.uint8), v_hist=json.dumps(hist))
    reads = argv[argv.index("-r") + 1]
    return path, d, argv, os.path.join(d, reads), {"first_run_s": round(dt, 2), "guarded_run_s": round(dt_g, 2), "guard_info": info[0] if info else None}


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
    ap.add_argument("--spans-only")
    ap.add_argument("--reads")
    ap.add_argument("--min-count", action="store_true", help="the set counts, and both calls are timed at t = 1, t = 2 and the valley (hypo --qv-min-count)")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--wall-runs", type=int, default=10)
    ap.add_argument("--parent-bin", help="hypo of a build of the parent commit (flag-off comparison)")
    args = ap.parse_args()
    if args.spans_only:
        print(json.dumps(spans_calls(args.spans_only, args.reads, args.min_count)))
        return
    out = os.path.abspath(args.out)
    os.makedirs(out, exist_ok=True)
    work = tempfile.mkdtemp(prefix="guard_rate_")
    res = {"what": f"hypo --kmer-guard, k = {K}, BASELINE config C3 (100 x 1 Mbp, 30x 150-bp reads)"}

    def save():
        json.dump(res, open(os.path.join(out, "guard_rate.json"), "w"), indent=1)
    path, d, argv, reads, res["run"] = prepare(work, args.threads)
    print(json.dumps(res["run"]), flush=True)
    child = [sys.executable, os.path.abspath(__file__), "--spans-only", path, "--reads", reads] + (["--min-count"] if args.min_count else [])
    p = subprocess.run(["timeout", "-k", "10", "600"] + child, capture_output=True, text=True)
    if p.returncode != 0:                                  # (nothing more on the GPU after a failed child)
        print(p.stderr[-1500:], flush=True)
        shutil.rmtree(work, ignore_errors=True)
        raise SystemExit(1)
    res["entry"] = json.loads(p.stdout.strip().splitlines()[-1])
    print(json.dumps(res["entry"]), flush=True)
    save()
    pdir = os.path.join(out, "rocprof_guard")
    p = subprocess.run(["timeout", "-k", "10", "600", "rocprofv3", "--kernel-trace", "--stats", "-d", pdir, "-o", "guard", "--output-format", "csv", "--"] + child,
                       capture_output=True, text=True)
    per_call = {}
    for root, _, files in os.walk(pdir):
        for f in files:
            if f.endswith("kernel_stats.csv"):
                for row in csv.DictReader(open(os.path.join(root, f))):
                    if "kset_" in row["Name"]:
                        calls = int(row["Calls"])
                        per_call[row["Name"].split("(")[0].replace("void hypo::", "")] = {
                            "calls": calls, "ms_per_call": round(float(row["TotalDurationNs"]) / calls / 1e6, 3)}
    res["rocprof_rc"] = p.returncode
    res["kernels"] = per_call
    print(json.dumps(per_call), flush=True)
    save()
    if p.returncode != 0:
        print(p.stderr[-1500:], flush=True)
        shutil.rmtree(work, ignore_errors=True)
        raise SystemExit(1)
    # wall time on C3: alternated
    kinds = {"no_flag": (argv, []), "qv": (argv, ["--qv", "t.tsv"]), "qv_guard": (argv, ["--qv", "t.tsv", "--kmer-guard"]),
             "guard": (argv, ["--kmer-guard"]), "guard_records": (argv, ["--guard-records"])}
    if args.parent_bin:
        kinds["no_flag_parent"] = ([os.path.abspath(args.parent_bin)] + argv[1:], [])
    runs = {k: [] for k in kinds}
    for i in range(args.wall_runs):
        for kind, (base, extra) in kinds.items():
            runs[kind].append(wall(base + extra, d)[0])
        print("wall", i, {k: round(v[-1], 3) for k, v in runs.items()}, flush=True)
    res["c3_wall"] = {k: spread(v) for k, v in runs.items()}
    res["c3_wall"]["guard_over_qv_median_pct"] = round(100 * (np.median(runs["qv_guard"]) / np.median(runs["qv"]) - 1), 2)
    res["c3_wall"]["guard_records_over_guard_median_pct"] = round(100 * (np.median(runs["guard_records"]) / np.median(runs["guard"]) - 1), 2)
    if args.parent_bin:
        res["c3_wall"]["no_flag_vs_parent_median_pct"] = round(100 * (np.median(runs["no_flag"]) / np.median(runs["no_flag_parent"]) - 1), 2)
    print(json.dumps(res["c3_wall"]), flush=True)
    shutil.rmtree(work, ignore_errors=True)
    save()


if __name__ == "__main__":
    main()
