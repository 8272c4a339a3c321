#!/usr/bin/env python3
"""The C2 step of bench.py on its own: the scan of one 5 Mbp contig at k = 11 plus the plan and POA of 97 078 C1-shaped windows,
two resident batches alternating, timed the way bench.py times its headline (warm-ups, fence, `steps` steps, fence).

usage: c2_step.py [--profile on|off|both] [--steps 20] [--warmup 3] [--repeats 5] [--windows 97078] [--lib libhypo_gpu.so] [--once]

--profile on   hypo_gpu_profile_begin is called before the timed steps (what bench.py does): every call records its kernels' times
--profile off  it is not: the step as `hypo` itself runs it
--profile both each repeat measures off, then on (default): their difference is what the profile records cost
--once         one pass of warm-ups + steps with profiling on, for a rocprofv3 --kernel-trace run of its own (prints the profile's means)
Prints one JSON line: ms_per_step of every repeat, medians, and with profiling on the mean profile_read values of the last repeat."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from hypo_amd import capi, sim  # noqa: E402

CONTIG_BASES, K = 5_000_000, 11          # bench.py: CONTIG_BASES, K


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profile", choices=["on", "off", "both"], default="both")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--windows", type=int, default=97078)
    ap.add_argument("--lib", default=capi.LIB_PATH)
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    gpu = capi.HypoGpu(0, path=args.lib)
    codes, packed4 = sim.random_contig(CONTIG_BASES, seed=2000, n_frac=0.0)
    bits = sim.solid_bitset(codes, K)
    ds = gpu.device_scan(packed4, CONTIG_BASES, K, bits, kids_cap=CONTIG_BASES // 2)
    batches = []
    for seed in (1000, 5000):
        b = sim.window_batch(args.windows, seed=seed)
        batches.append(gpu.device_batch(b, off=b.slot_layout()))
    step_no = [0]

    def step():
        ds.run()
        batches[step_no[0] % 2].run()
        step_no[0] += 1

    def measure(profiled):
        step_no[0] = 0
        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize(dev)
        gpu.profile_begin(min(256, 2 * args.steps) if profiled else 0)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize(dev)
        dt = (time.perf_counter() - t0) / args.steps
        prof = gpu.profile_read() if profiled else []
        gpu.profile_begin(0)
        return dt * 1e3, prof

    def kernel_means(prof):
        out = {}
        poa = [p for p in prof if len(p) == 8]
        scan = [p for p in prof if len(p) == 3]
        if poa:
            out["poa_kernels_ms"] = [round(sum(p[i] for p in poa) / len(poa), 4) for i in range(8)]
        if scan:
            out["scan_kernels_ms"] = [round(sum(p[i] for p in scan) / len(scan), 4) for i in range(3)]
        return out

    if args.once:                                         # (under the tracer: the profile's values of the very calls it traces)
        t, prof = measure(True)
        print(json.dumps({"script": "c2_step --once", "lib": os.path.basename(args.lib), "ms_per_step": round(t, 4), **kernel_means(prof)}))
        return
    modes = ["off", "on"] if args.profile == "both" else [args.profile]
    ms = {m: [] for m in modes}
    prof = []
    for _ in range(args.repeats):
        for m in modes:
            t, p = measure(m == "on")
            ms[m].append(round(t, 4))
            prof = p or prof
    out = {"script": "c2_step", "lib": os.path.basename(args.lib), "build_id": gpu.lib.hypo_gpu_build_id().decode(),
           "steps": args.steps, "warmup": args.warmup, "windows": args.windows,
           "ms_per_step": ms, "median_ms": {m: round(statistics.median(v), 4) for m, v in ms.items()}}
    if len(modes) == 2:
        out["profile_cost_ms"] = round(out["median_ms"]["on"] - out["median_ms"]["off"], 4)
    out.update(kernel_means(prof))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
