#!/usr/bin/env python3
"""hypo --qv-save / --qv-load on the MI355X: what building the k-mer set from the reads costs against taking it from a file, and what
the two flags leave of a run without them (DESIGN.md "k-mer set file").

    python profiles/setfile_rate.py --out DIR [--parent-bin PATH]        # everything below, in one call
      1. 30x reads of a 5 Mbp genome (profiles/gen_reads.py) are written to a scratch directory.  A child builds a counting 21-mer
         set from the file's bytes through hypo_gpu_kset_add in 256 MiB calls (the parent commit's path; without the parse), and a
         set that does not count likewise; runs export sequences with a buffer of 2^24 records (records/s, best of 3, the first
         sequence apart), next to a plain device-to-host copy of as many bytes; writes the records with numpy in the file's layout
         and reads them back (what the disk takes); and imports them into a fresh set in calls of 2^24 records.  BASELINE config C3
         has no reads, hence no k-mer: no rate is taken from it.
      2. e2e_real_5m_s131 (5 x 1 Mbp, stage 1 over its stored solid k-mers) is generated, its reads file is replaced by the reads of
         step 1 (another genome: what is timed is how the set is made, not what it says), and `hypo --qv` runs --wall-runs
         alternated times (default 5; process wall): the set built from the reads, built and saved, and loaded from the saved
         file.  The seconds of the `saved` and `loaded` Info lines are hypo's own export + write and read + import.
      3. e2e_c3_100m_s31 (100 x 1 Mbp, -p 10): `hypo` without a flag, --wall-runs alternated runs each, this build and the parent
         commit's (--parent-bin: hypo of a build of the parent, beside its two libraries).
    python profiles/setfile_rate.py --entry-only READS                   # (the child of step 1)
Every step that uses the GPU is a child under a time limit of its own; after one that fails nothing more is started."""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
K = 21
GENOME = 5_000_000
PIECE = 256 << 20
CAP = 1 << 24


def insert_all(gpu, data):
    t, at = 0.0, 0
    while True:
        t0 = time.perf_counter()
        gpu.kset_add(data[at:at + PIECE])
        t += time.perf_counter() - t0
        if at + PIECE >= data.size:
            return t
        at += PIECE - (K - 1)


def entry_calls(reads, scratch):
    import torch
    from hypo_amd import capi
    gpu = capi.HypoGpu(0)
    data = np.fromfile(reads, dtype=np.uint8)
    out = {"k": K, "reads_file_GB": round(data.size / 1e9, 3)}
    gpu.kset_begin(K, GENOME)
    out["build_plain_add_calls_s"] = round(insert_all(gpu, data), 4)
    gpu.kset_end()
    gpu.kset_begin(K, GENOME)
    gpu.kset_counts_enable(1)
    out["build_counting_add_calls_s"] = round(insert_all(gpu, data), 4)
    n, table_bytes = gpu.kset_size()
    out.update({"distinct": n, "resident_GiB": round(table_bytes / 2 ** 30, 3)})
    # the entry itself, into two buffers allocated once
    import ctypes as C
    keys, counts = np.empty(n + CAP, np.uint64), np.empty(n + CAP, np.uint8)         # (room for a whole call behind the last record)
    ts = []
    for _ in range(4):                                       # the first sequence grows the arenas
        cursor, got, digest, n_outs = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), []
        at = 0
        t0 = time.perf_counter()
        while cursor.value != 0xFFFFFFFFFFFFFFFF:
            rc = gpu.lib.hypo_gpu_kset_export(C.byref(cursor), C.c_void_p(keys.ctypes.data + 8 * at), C.c_void_p(counts.ctypes.data + at), C.c_uint64(CAP),
                                              C.byref(got), C.byref(digest))
            assert rc == 0, gpu.lib.hypo_gpu_last_error()
            at += got.value
            n_outs.append(got.value)
        ts.append(time.perf_counter() - t0)
    assert at == n
    keys, counts, digest = keys[:n], counts[:n], digest.value
    t0 = time.perf_counter()
    k_b, c_b, d_b, _ = gpu.kset_export(CAP)
    out["export_through_the_binding_s"] = round(time.perf_counter() - t0, 4)
    assert np.array_equal(k_b, keys) and np.array_equal(c_b, counts) and d_b == digest
    dev = torch.empty(n * 9, dtype=torch.uint8, device="cuda")
    tc = []
    for _ in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dev.cpu()
        tc.append(time.perf_counter() - t0)
    out["export"] = {"calls": len(n_outs), "first_s": round(ts[0], 4), "sequence_s": [round(t, 4) for t in ts[1:]], "best_s": round(min(ts[1:]), 4),
                     "records_per_s": round(n / min(ts[1:])), "plain_copy_of_as_many_bytes_s": round(min(tc[1:]), 4),
                     "copy_share": round(min(tc[1:]) / min(ts[1:]), 3)}
    gpu.kset_end()
    # the disk: the records in the file's layout, one block (hypo's own writer and reader are timed in step 2)
    path = os.path.join(scratch, "records.hks")
    t0 = time.perf_counter()
    with open(path, "wb") as f:
        f.write(b"HYPOKSET" + np.array([1, K], "<u4").tobytes() + np.array([n, n], "<u8").tobytes())
        keys.tofile(f)
        counts.tofile(f)
        f.write(b"\0" * (-n % 8) + np.array([0, digest], "<u8").tobytes())
        f.flush()
        os.fsync(f.fileno())
    out["file"] = {"bytes": os.path.getsize(path), "write_fsync_s": round(time.perf_counter() - t0, 4)}
    t0 = time.perf_counter()
    with open(path, "rb") as f:
        f.seek(32)
        k2 = np.fromfile(f, "<u8", n)
        c2 = np.fromfile(f, "u1", n)
    out["file"]["read_s"] = round(time.perf_counter() - t0, 4)
    for name, counting in (("import_counting", True), ("import_plain", False)):
        gpu.kset_begin(K, n)
        if counting:
            gpu.kset_counts_enable(1)
        t0 = time.perf_counter()
        d = 0
        for at in range(0, n, CAP):
            d = (d + gpu.kset_import(k2[at:at + CAP], c2[at:at + CAP])) & 0xFFFFFFFFFFFFFFFF
        dt = time.perf_counter() - t0
        assert d == digest and gpu.kset_size()[0] == n
        out[name] = {"s": round(dt, 4), "records_per_s": round(n / dt)}
        gpu.kset_end()
    os.remove(path)
    return out


def wall(argv, cwd):
    env = dict(os.environ, HYPO_REQUIRE_DEVICE="1")
    t0 = time.perf_counter()
    p = subprocess.run(["timeout", "-k", "10", "300"] + argv, cwd=cwd, env=env, capture_output=True, text=True)
    dt = time.perf_counter() - t0
    if p.returncode != 0:
        raise SystemExit(f"hypo failed ({p.returncode}): {p.stderr[-1500:]}")
    return dt, p.stdout, p.stderr


def spread(ts):
    ts = np.array(ts)
    return {"runs_s": [round(float(t), 3) for t in ts], "median_s": round(float(np.median(ts)), 3), "min_s": round(float(ts.min()), 3),
            "max_s": round(float(ts.max()), 3), "std_s": round(float(ts.std(ddof=1)), 3) if ts.size > 1 else 0.0}


def fast_set(eu, work, name, threads):
    d = os.path.join(work, "set_" + name)
    os.makedirs(d)
    man, p, dt, _ = eu.run_fast_case(name, d, threads=threads)
    argv = [eu.BIN] + man["command"].split()[1:]
    if "our_p" in man["args"] and "-p" in argv:
        argv[argv.index("-p") + 1] = str(man["args"]["our_p"])
    argv[argv.index("-t") + 1] = str(threads)
    return d, argv, dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--entry-only")
    ap.add_argument("--scratch")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--wall-runs", type=int, default=5)
    ap.add_argument("--parent-bin", help="hypo of a build of the parent commit (flag-off comparison)")
    ap.add_argument("--skip-c3", action="store_true")
    args = ap.parse_args()
    if args.entry_only:
        print(json.dumps(entry_calls(args.entry_only, args.scratch or os.path.dirname(args.entry_only))))
        return
    import e2e_util as eu
    import gen_reads
    out = os.path.abspath(args.out)
    os.makedirs(out, exist_ok=True)
    res = {"what": f"hypo --qv-save / --qv-load, k = {K}: 30x reads of a {GENOME // 10 ** 6} Mbp genome; the flags on e2e_real_5m_s131 with those reads; no flag on BASELINE config C3 against the parent"}

    def save():
        json.dump(res, open(os.path.join(out, "setfile_rate.json"), "w"), indent=1)
    work = tempfile.mkdtemp(prefix="setfile_rate_")
    reads = os.path.join(work, "reads_5m.fa")
    gen_reads.generate(reads, GENOME)
    p = subprocess.run(["timeout", "-k", "10", "400", sys.executable, os.path.abspath(__file__), "--entry-only", reads, "--scratch", work], capture_output=True, text=True)
    if p.returncode != 0:                                  # (nothing more on the GPU after a failed child)
        print(p.stdout[-1500:], p.stderr[-1500:], flush=True)
        raise SystemExit(1)
    res["entry"] = json.loads(p.stdout.strip().splitlines()[-1])
    print(json.dumps(res["entry"]), flush=True)
    save()

    # step 2: the flags on a 5 Mbp run
    d, argv, dt = fast_set(eu, work, "e2e_real_5m_s131", args.threads)
    shutil.copyfile(reads, os.path.join(d, argv[argv.index("-r") + 1]))
    kinds = {"built": ["--qv", "q.tsv"], "built_and_saved": ["--qv", "q.tsv", "--qv-save", "s.hks"], "loaded": ["--qv", "q.tsv", "--qv-load", "s.hks"]}
    wall(argv + kinds["built_and_saved"], d)                # (the file of the first `loaded` run, and a warm page cache for everyone)
    runs = {k: [] for k in kinds}
    own = {"saved_s": [], "loaded_s": [], "insert_calls_s": []}
    for i in range(args.wall_runs):
        for kind, extra in kinds.items():
            dt, stdout, stderr = wall(argv + extra, d)
            runs[kind].append(dt)
            for key, pat, text in (("saved_s", r"k-mer set saved to .*, ([0-9.]+) s\)", stdout), ("loaded_s", r"k-mer set loaded from .*, ([0-9.]+) s\)", stdout),
                                   ("insert_calls_s", r"distinct k-mers, ([0-9.]+) s in the insert calls", stderr)):
                m = re.search(pat, text)
                if m and (key != "insert_calls_s" or kind == "built"):
                    own[key].append(float(m.group(1)))
        print("wall", i, {k: round(v[-1], 3) for k, v in runs.items()}, flush=True)
        res["real_5m_wall"] = {k: spread(v) for k, v in runs.items()}
        res["real_5m_wall"]["hypo_own_seconds"] = own
        res["real_5m_wall"]["file_bytes"] = os.path.getsize(os.path.join(d, "s.hks"))
        save()
    med = lambda r, k: float(np.median(r[k]))
    res["real_5m_wall"]["loaded_vs_built_median_pct"] = round(100 * (med(runs, "loaded") / med(runs, "built") - 1), 2)
    res["real_5m_wall"]["saved_vs_built_median_pct"] = round(100 * (med(runs, "built_and_saved") / med(runs, "built") - 1), 2)
    print(json.dumps(res["real_5m_wall"]), flush=True)
    save()
    shutil.rmtree(d, ignore_errors=True)

    # step 3: no flag on C3, this build and the parent's
    if not args.skip_c3:
        d, argv, dt = fast_set(eu, work, "e2e_c3_100m_s31", args.threads)
        kinds = {"no_flag": argv}
        if args.parent_bin:
            kinds["no_flag_parent"] = [os.path.abspath(args.parent_bin)] + argv[1:]
        runs = {k: [] for k in kinds}
        for i in range(args.wall_runs):
            for kind, a in kinds.items():
                runs[kind].append(wall(a, d)[0])
            print("c3", i, {k: round(v[-1], 3) for k, v in runs.items()}, flush=True)
            res["c3_wall"] = {k: spread(v) for k, v in runs.items()}
            save()
        if args.parent_bin:
            res["c3_wall"]["no_flag_vs_parent_median_pct"] = round(100 * (med(runs, "no_flag") / med(runs, "no_flag_parent") - 1), 2)
        print(json.dumps(res["c3_wall"]), flush=True)
    shutil.rmtree(work, ignore_errors=True)
    save()


if __name__ == "__main__":
    main()
