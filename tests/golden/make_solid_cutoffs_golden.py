#!/usr/bin/env python3
"""Cut-off fixtures: k-mer histogram -> {err, mean, lower, upper} of the REAL suk::SolidKmers::find_cutoffs
(external/suk/src/SolidKmers.cpp:258-363), compiled in place from the reference's sources together with the sdsl sources its
bit vector needs, by the recipe of oracle/Makefile's libhyporef_scan.so (hidden visibility, -ffunction-sections,
--gc-sections, -z defs: SolidKmers::initialise and its KMC calls are dropped, not stubbed), around
tests/golden/ref_cutoffs_harness.cpp.  Nothing of the reference is copied.

Run in the build container only (needs the reference tree; REF=<path> overrides its place):
    python tests/golden/make_solid_cutoffs_golden.py
Writes tests/golden/solid_cutoffs.json.gz: [{"name", "hist": [...], "result": [err, mean, lower, upper] | "undefined"}].

Cases: histograms counted by tests/solid_checker.py from gen_e2e read sets at k 7..17 and c 10..80; crafted shapes (plan B,
err_th > 100, ties, flat tails, upper == 4c); the same shapes scaled past 2^32 (the UINT truncations); random shapes.  Inputs
without a maximum after the error threshold are left out of the reference call (its mean would be unset) and recorded as
"undefined".
"""
import ctypes as C
import gzip
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import solid_checker as sc  # noqa: E402
import gen_e2e  # noqa: E402

R = os.environ.get("REF", "/root/reference")


def build_harness(out_dir):
    sdsl = f"{R}/external/sdsl-lite/lib"
    srcs = [f"{R}/external/suk/src/SolidKmers.cpp"] + [f"{sdsl}/{x}.cpp" for x in
                                                       ("bits", "memory_management", "ram_fs", "util", "io", "sfstream", "ram_filebuf")]
    inc = [f"-I{R}/include", f"-I{R}/external/sdsl-lite/include", f"-I{R}/external/suk/include", f"-I{R}/external/slog/include",
           f"-I{R}/external/suk/external/kmc_api"]
    so = os.path.join(out_dir, "libref_cutoffs.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-w", "-fopenmp", "-fPIC", "-shared", "-include", "stdexcept",
                           "-fvisibility=hidden", "-ffunction-sections", "-fdata-sections", "-Wl,--gc-sections", "-Wl,-z,defs",
                           *inc, "-o", so, os.path.join(HERE, "ref_cutoffs_harness.cpp"), *srcs, "-lz"])
    return C.CDLL(so)


def crafted(rng):
    out = []
    # plan B: a peak and then a strictly falling right side (every window of five is lower)
    for c, peak in ((10, 12), (30, 25), (40, 60), (80, 200)):
        h = np.zeros(4 * c + 1, dtype=np.uint64)
        for v in range(2, 4 * c + 1):
            h[v] = int(5000 * np.exp(-(v - 2) / 1.5) + 3000 * np.exp(-0.5 * ((v - peak) / (peak / 4)) ** 2) + (4 * c - v)) + 1
        for v in range(peak + 1, 4 * c + 1):
            h[v] = min(int(h[v]), int(h[v - 1]) - 1) if h[v - 1] > 1 else 1
        out.append((f"planB_c{c}", h))
    # err_th > 100: falling over more than 100 bins
    for c in (30, 40, 80):
        h = np.array([0, 0] + [10 ** 6 - 37 * v for v in range(2, 4 * c + 1)], dtype=np.uint64)
        h[4 * c - 5] += 10 ** 6
        out.append((f"errth_gt100_c{c}", h))
    # ties and flat tails
    for c in (10, 30):
        h = np.zeros(4 * c + 1, dtype=np.uint64)
        h[2:6] = [900, 500, 200, 200]
        h[6:4 * c + 1] = 300
        h[c] = 700
        out.append((f"flat_tail_c{c}", h.copy()))
        h[c + 1] = 700
        out.append((f"tie_at_max_c{c}", h.copy()))
        h2 = np.zeros(4 * c + 1, dtype=np.uint64)
        h2[2] = 50
        h2[3:4 * c + 1] = 40
        out.append((f"all_flat_c{c}", h2))
    # upper == 4c: the maximum right before the last bin
    for c in (10, 30):
        h = np.zeros(4 * c + 1, dtype=np.uint64)
        h[2:5] = [1000, 400, 100]
        for v in range(5, 4 * c + 1):
            h[v] = 100 + 30 * v
        out.append((f"upper_is_4c_c{c}", h))
        h = h.copy()
        h[4 * c - 1] = 5000
        out.append((f"mean_at_4c_minus1_c{c}", h))
    # undefined: nothing after the error threshold
    out.append(("undefined_zero_tail", np.array([0, 0, 5, 3, 1] + [0] * 36, dtype=np.uint64)))
    out.append(("undefined_all_zero", np.zeros(41, dtype=np.uint64)))
    out.append(("undefined_falling", np.array([0, 0] + list(range(39, 0, -1)), dtype=np.uint64)))
    # bins above 2^32 (UINT global_maxima_val, the wrapping delta_sum and the truncated quotient)
    big = []
    for name, h in out:
        for s in (1 << 32, (1 << 33) + 12345, 1 << 40):
            big.append((f"{name}_x{s}", (h.astype(object) * s + rng.integers(0, 1 << 20, size=h.size).astype(object) *
                                         (h > 0).astype(object)).astype(object)))
    # a bin that truncates to less than its neighbours as a UINT
    h = np.zeros(121, dtype=object)
    h[2:5] = [10 ** 12, 10 ** 11, 10 ** 10]
    for v in range(5, 121):
        h[v] = 1000 + 10 * v
    h[30] = (1 << 32) + 5
    h[31] = (1 << 32) - 7
    big.append(("truncation_c30", h))
    return out + big


def random_shapes(rng, n):
    out = []
    for i in range(n):
        c = int(rng.integers(3, 90))
        top = 4 * c
        v = np.arange(top + 1)
        mean = rng.uniform(1, top * 0.9)
        sd = rng.uniform(0.5, max(1.0, mean / 2))
        err = rng.uniform(0, 10 ** rng.uniform(2, 7))
        h = err * np.exp(-v / rng.uniform(0.3, 4)) + rng.uniform(10, 10 ** rng.uniform(2, 7)) * np.exp(-0.5 * ((v - mean) / sd) ** 2)
        h = h * rng.uniform(0.8, 1.2, size=h.size) + rng.integers(0, 5, size=h.size)
        if rng.random() < 0.3:
            h = np.round(h / 10) * 10                 # ties
        h = h.astype(np.int64).astype(object)
        if rng.random() < 0.2:
            h = h * (1 << int(rng.integers(30, 40)))
        h[0] = h[1] = 0
        out.append((f"random_{i}", h))
    return out


def from_reads(tmp):
    out = []
    for seed, G in ((1, 20000), (5, 60000)):
        d = os.path.join(tmp, f"s{seed}")
        gen_e2e.generate(d, seed, G, False, K=5)
        seqs = sc.parse_records([os.path.join(d, "reads.fa")])
        for k in (7, 9, 11, 13, 15, 17):
            codes, counts = sc.count_canonical(seqs, k)
            for c in (10, 15, 30, 45, 80):
                out.append((f"reads_s{seed}_G{G}_k{k}_c{c}", sc.histogram(counts, c)))
    return out


def main():
    rng = np.random.default_rng(2026)
    with tempfile.TemporaryDirectory() as tmp:
        lib = build_harness(tmp)
        cases = from_reads(tmp) + crafted(rng) + random_shapes(rng, 400)
        rows = []
        n_undef = 0
        for name, h in cases:
            hl = [int(x) for x in h]
            if sc.find_cutoffs(hl) is None:
                rows.append({"name": name, "hist": hl, "result": "undefined"})
                n_undef += 1
                continue
            arr = (C.c_uint64 * len(hl))(*[x & 0xFFFFFFFFFFFFFFFF for x in hl])
            out = (C.c_uint32 * 4)()
            lib.hyporef_find_cutoffs(arr, C.c_uint32(len(hl)), out)
            rows.append({"name": name, "hist": hl, "result": [int(x) for x in out]})
    path = os.path.join(HERE, "solid_cutoffs.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps(rows, separators=(",", ":")).encode())
    print(f"wrote {path}: {len(rows)} cases, {n_undef} undefined")


if __name__ == "__main__":
    main()
