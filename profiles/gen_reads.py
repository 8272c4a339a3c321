#!/usr/bin/env python3
"""Large short-read sets for profiles/solid_rate.py: a random genome, 150-bp reads from both strands at 30x, 0.2 % substitutions,
about one N per 2 000 bases; FASTA, one header ">r" per read.  Written in blocks of a million reads with numpy.
    python profiles/gen_reads.py <out.fa> <genome bases> [--cov 30] [--seed 1]"""
import argparse

import numpy as np

COMP = np.frombuffer(b"TGCA", dtype=np.uint8)


def generate(path, G, cov=30, seed=1, read_len=150, sub=0.002, n_rate=0.0005):
    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(b"ACGT", dtype=np.uint8)
    codes = rng.integers(0, 4, G, dtype=np.uint8)
    n_reads = G * cov // read_len
    with open(path, "wb") as f:
        for at in range(0, n_reads, 1 << 20):
            n = min(1 << 20, n_reads - at)
            starts = rng.integers(0, G - read_len + 1, n)
            r = codes[starts[:, None] + np.arange(read_len)]
            m = rng.random(r.shape) < sub
            r[m] = (r[m] + rng.integers(1, 4, int(m.sum()), dtype=np.uint8)) & 3
            rev = rng.random(n) < 0.5
            r[rev] = (3 - r[rev])[:, ::-1]
            seq = alphabet[r]
            seq[rng.random(seq.shape) < n_rate] = ord("N")
            rows = np.empty((n, 3 + read_len + 1), dtype=np.uint8)
            rows[:, :3] = np.frombuffer(b">r\n", dtype=np.uint8)
            rows[:, 3:3 + read_len] = seq
            rows[:, -1] = ord("\n")
            f.write(rows.tobytes())
    return n_reads * read_len


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("G", type=int)
    ap.add_argument("--cov", type=int, default=30)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    print(generate(a.out, a.G, a.cov, a.seed))
