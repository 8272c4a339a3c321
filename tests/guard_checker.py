"""CPU checker of `hypo --kmer-guard` (DESIGN.md "k-mer guard"): the contract in plain Python / numpy.  It shares no code with the
host library or the kernels; the k-mer arithmetic is qv_checker's, the records are edit_checker's.

Terms: k the k-mer length, R the read set (qv_checker.read_set), D a draft contig as PackedSeq::base_at gives it
(qv_checker.draft_text), recs its VCF records [(pos1, ref, alt, info)] (edit_checker.records / parse_vcf), P = apply(recs, D).

  clusters(recs, k)        [(i0, i1, b, e, qb, qe)]: records [i0, i1) form a cluster; consecutive records share one when fewer than
                           k - 1 unchanged draft bases separate them (b_{i+1} - e_i < k - 1).  [b, e) is its draft span, [qb, qe)
                           the same span in P.  The whole-contig <DEL> record forms no cluster.
  spans(D, P, c, k)        (ref, alt): the two spans with up to k - 1 bases on either side
  guard(D, recs, k, R)     Result: per record "PASS" / "kmer", the guarded text, the counts of the stdout line, (r_c, a_c) per cluster.
                           A cluster is rejected when a_c > r_c (a tie trusts the polish); a rejected cluster rejects all its records.
  info_line(k, results)    the stdout line of a run, from the results of its contigs
"""
from collections import namedtuple

import edit_checker as ec
import qv_checker as qc

FILTER_HEADER = '##FILTER=<ID=kmer,Description="rejected: adds k-mers that no read contains">'
Result = namedtuple("Result", "filters text n_clusters n_records rej_clusters rej_records scores clusters")


def is_whole_del(recs):
    return len(recs) == 1 and recs[0][2] == "<DEL>"


def clusters(recs, k):
    if is_whole_del(recs):
        return []
    out, shift = [], 0
    for i, (pos, ref, alt, _) in enumerate(recs):
        b, e = pos - 1, pos - 1 + len(ref)
        if out and b - out[-1][3] < k - 1:
            i0, _, cb, _, qb, _ = out.pop()
        else:
            i0, cb, qb = i, b, b + shift
        shift += len(alt) - len(ref)
        out.append((i0, i + 1, cb, e, qb, e + shift))
    return out


def spans(D, P, c, k):
    _, _, b, e, qb, qe = c
    return D[max(0, b - k + 1):min(len(D), e + k - 1)], P[max(0, qb - k + 1):min(len(P), qe + k - 1)]


def missing(seq, k, R):
    return qc.seq_stats(seq, k, R)[1]


def guard(D, recs, k, R):
    P = ec.apply(recs, D)
    cl = clusters(recs, k)
    filters = ["PASS"] * len(recs)
    scores = []
    rej_c = rej_r = 0
    for c in cl:
        ref, alt = spans(D, P, c, k)
        r_c, a_c = missing(ref, k, R), missing(alt, k, R)
        scores.append((r_c, a_c))
        if a_c > r_c:
            rej_c += 1
            rej_r += c[1] - c[0]
            for i in range(c[0], c[1]):
                filters[i] = "kmer"
    text = ec.apply([r for r, f in zip(recs, filters) if f == "PASS"], D)
    return Result(filters, text, len(cl), sum(c[1] - c[0] for c in cl), rej_c, rej_r, scores, cl)


def info_line(k, results):
    s = [sum(getattr(r, f) for r in results) for f in ("n_clusters", "n_records", "rej_clusters", "rej_records")]
    return f"[Hypo::Hypo] Info: k-mer guard (k = {k}): {s[0]} clusters of {s[1]} records, {s[2]} clusters ({s[3]} records) rejected"


def parse_vcf_filters(text):
    """{contig: [FILTER]} in file order, and the header lines"""
    head, out = [], {}
    for l in text.splitlines():
        if l.startswith("#"):
            head.append(l)
            continue
        f = l.split("\t")
        out.setdefault(f[0], []).append(f[6])
    return head, out
