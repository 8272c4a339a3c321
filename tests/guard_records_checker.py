"""CPU checker of `hypo --guard-records` (DESIGN.md "k-mer guard by record"): the contract in plain Python on top of guard_checker,
edit_checker and qv_checker.  It shares no code with the host library or the kernels.

Terms are guard_checker's: k, R, D, recs, clusters(recs, k).  N is the limit on records per cluster.

  variant_text(D, recs, c, mask, k)   the text of the subset `mask` of cluster c's records (bit j = record i0 + j): up to k - 1 draft
                                      bases, D[b:e] with the subset applied, up to k - 1 draft bases
  choose(D, recs, c, k, R)            (mask, miss(mask), [miss(m) for every m]): fewest missing, then most records, then greatest mask
  guard(D, recs, k, R, N)             Result: per record "PASS" / "kmer", the guarded text, the counts of the stdout line, per cluster
                                      (miss(none), miss(chosen)), the chosen masks (None where the cluster was decided whole)
  info_line(k, N, results)            the stdout line of a run
  site_variants(data, alts, lo, hi, edits)   the strings of all 2^n variants of one site of hypo_gpu_kset_query_variants
  best(pairs)                         the index the entry point must name among (total, missing) pairs in mask order
"""
from collections import namedtuple

import edit_checker as ec
import guard_checker as gc

Result = namedtuple("Result", "filters text n_clusters n_records rej_whole rej_part rej_records scores masks clusters sizes")


def variant_text(D, recs, c, mask, k):
    i0, i1, b, e = c[:4]
    out, at = [D[max(0, b - k + 1):b]], b
    for j, (pos, ref, alt, _) in enumerate(recs[i0:i1]):
        rb = pos - 1
        assert rb >= at and D[rb:rb + len(ref)] == ref
        if (mask >> j) & 1:
            out += [D[at:rb], alt]
            at = rb + len(ref)
    assert at <= e
    out += [D[at:e], D[e:min(len(D), e + k - 1)]]
    return "".join(out)


def best(missing):
    """the index of the chosen variant among the missing counts in mask order"""
    return max(range(len(missing)), key=lambda m: (-missing[m], bin(m).count("1"), m))


def choose(D, recs, c, k, R):
    n = c[1] - c[0]
    miss = [gc.missing(variant_text(D, recs, c, m, k), k, R) for m in range(1 << n)]
    m = best(miss)
    return m, miss[m], miss


def guard(D, recs, k, R, N):
    cl = gc.clusters(recs, k)
    filters = ["PASS"] * len(recs)
    scores, masks, sizes = [], [], {}
    whole = part = rej_r = 0
    for c in cl:
        n = c[1] - c[0]
        sizes[n if n <= N else 0] = sizes.get(n if n <= N else 0, 0) + 1
        full = (1 << n) - 1
        if n == 1 or n > N:                      # guard_checker's decision: the whole cluster, rejected iff a_c > r_c
            r_c, a_c = (gc.missing(variant_text(D, recs, c, m, k), k, R) for m in (0, full))
            m = 0 if a_c > r_c else full
            scores.append((r_c, r_c if m == 0 else a_c))
            masks.append(None)
        else:
            m, got, miss = choose(D, recs, c, k, R)
            scores.append((miss[0], got))
            masks.append(m)
        rejected = [c[0] + j for j in range(n) if not (m >> j) & 1]
        for i in rejected:
            filters[i] = "kmer"
        rej_r += len(rejected)
        whole += len(rejected) == n
        part += 0 < len(rejected) < n
    text = ec.apply([r for r, f in zip(recs, filters) if f == "PASS"], D)
    return Result(filters, text, len(cl), sum(c[1] - c[0] for c in cl), whole, part, rej_r, scores, masks, cl, sizes)


def info_line(k, N, results):
    s = [sum(getattr(r, f) for r in results) for f in ("n_clusters", "n_records", "rej_whole", "rej_part", "rej_records")]
    return (f"[Hypo::Hypo] Info: k-mer guard (k = {k}, by record in clusters of up to {N}): {s[0]} clusters of {s[1]} records, "
            f"{s[2]} clusters rejected whole, {s[3]} in part, {s[4]} records rejected")


def site_variants(data, alts, lo, hi, edits):
    """edits: [(eb, ee, ao, al)] of one site data[lo:hi].  The byte strings of its 2^n variants in mask order."""
    out = []
    for m in range(1 << len(edits)):
        parts, at = [], lo
        for j, (b, e, ao, al) in enumerate(edits):
            assert at <= b <= e <= hi
            parts.append(data[at:b])
            parts.append(alts[ao:ao + al] if (m >> j) & 1 else data[b:e])
            at = e
        parts.append(data[at:hi])
        out.append(b"".join(parts))
    return out
