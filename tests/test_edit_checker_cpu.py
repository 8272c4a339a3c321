"""The edit-script checker (tests/edit_checker.py) against brute force and the properties the contract promises."""
import itertools
import random

import edit_checker as ec


def all_alignments(a, b):
    """every alignment of a against b as an op string (exhaustive)"""
    if not a and not b:
        yield ""
        return
    if a and b:
        for r in all_alignments(a[:-1], b[:-1]):
            yield r + ("=" if a[-1] == b[-1] else "X")
    if a:
        for r in all_alignments(a[:-1], b):
            yield r + "D"
    if b:
        for r in all_alignments(a, b[:-1]):
            yield r + "I"


def cost(ops):
    return sum(o != "=" for o in ops)


def check_script(a, b, ops):
    """ops is an alignment of a against b"""
    i = j = 0
    for o in ops:
        if o in "=X":
            assert (a[i] == b[j]) == (o == "="), (a, b, ops)
            i += 1
            j += 1
        elif o == "D":
            i += 1
        else:
            j += 1
    assert i == len(a) and j == len(b)


def canonical_brute(a, b):
    """the traceback of the contract from the full matrix, recursively (first move that holds: diagonal, up, left)"""
    n, m = len(a), len(b)
    D = [[0] * (m + 1) for _ in range(n + 1)]
    for i in range(n + 1):
        for j in range(m + 1):
            if i == 0 or j == 0:
                D[i][j] = i + j
            else:
                D[i][j] = min(D[i - 1][j - 1] + (a[i - 1] != b[j - 1]), D[i - 1][j] + 1, D[i][j - 1] + 1)
    ops, i, j = [], n, m
    while i or j:
        if i and j and D[i][j] == D[i - 1][j - 1] + (a[i - 1] != b[j - 1]):
            ops.append("=" if a[i - 1] == b[j - 1] else "X")
            i, j = i - 1, j - 1
        elif i and D[i][j] == D[i - 1][j] + 1:
            ops.append("D")
            i -= 1
        else:
            ops.append("I")
            j -= 1
    return D[n][m], "".join(reversed(ops))


def strings(alpha, up_to):
    for n in range(up_to + 1):
        for t in itertools.product(alpha, repeat=n):
            yield "".join(t)


def test_distance_and_script_exhaustive_acg_up_to_4():
    ss = list(strings("ACG", 4))
    for a in ss:
        for b in ss:
            d, ops = ec.align(a.encode(), b.encode())
            assert d == min(cost(x) for x in all_alignments(a, b)), (a, b)
            check_script(a, b, ops)
            assert cost(ops) == d
            assert (d, ops) == canonical_brute(a, b), (a, b)


def test_random_pairs_match_recursive_traceback():
    rnd = random.Random(5)
    for _ in range(300):
        a = "".join(rnd.choice("ACGTN") for _ in range(rnd.randint(0, 40)))
        b = list(a)
        for _ in range(rnd.randint(0, 8)):
            k = rnd.randint(0, 2)
            p = rnd.randint(0, len(b))
            if k == 0 and p < len(b):
                b[p] = rnd.choice("ACGT")
            elif k == 1 and p < len(b):
                del b[p]
            else:
                b.insert(p, rnd.choice("ACGT"))
        b = "".join(b)
        assert ec.align(a.encode(), b.encode()) == canonical_brute(a, b)


def test_suffix_trim_is_exact_prefix_trim_is_not():
    rnd = random.Random(7)
    for _ in range(300):
        a = "".join(rnd.choice("AC") for _ in range(rnd.randint(0, 10)))
        b = "".join(rnd.choice("AC") for _ in range(rnd.randint(0, 10)))
        s = rnd.choice("AC") * rnd.randint(1, 3)
        d, ops = ec.align((a + s).encode(), (b + s).encode())
        d2, ops2 = ec.align(a.encode(), b.encode())
        assert d == d2 and ops == ops2 + "=" * len(s)
    # the counterexample of the contract: AA vs A deletes the FIRST A (trimming the common prefix would delete the second)
    assert ec.align(b"AA", b"A") == (1, "D=")
    assert ec.align(b"A", b"A") == (0, "=")


def test_indels_leftmost_in_homopolymers_and_repeats():
    assert ec.align(b"CAAAAG", b"CAAAG")[1] == "=D===="
    assert ec.align(b"CAAAG", b"CAAAAG")[1] == "=I===="
    assert ec.align(b"TACACACG", b"TACACG")[1] == "=DD====="
    assert ec.align(b"TACACG", b"TACACACG")[1] == "=II====="


def rand_seq(rnd, n):
    return "".join(rnd.choice("ACGT") for _ in range(n))


def mutate(rnd, s, n_edits):
    s = list(s)
    for _ in range(n_edits):
        k = rnd.randint(0, 2)
        p = rnd.randint(0, len(s))
        if k == 0 and p < len(s):
            s[p] = rnd.choice("ACGT")
        elif k == 1 and p < len(s):
            del s[p]
        else:
            s.insert(p, rnd.choice("ACGT"))
    return "".join(s)


def build(draft, spans):
    """units and the output of a draft with [b, e) -> text replacements"""
    units, out, at = [], [], 0
    for b, e, t in spans:
        out.append(draft[at:b])
        out.append(t)
        _, ops = ec.align(draft[b:e].encode(), t.encode())
        units.append((b, e, t, ec.runs(ops)))
        at = e
    out.append(draft[at:])
    return units, "".join(out)


def roundtrip(draft, spans):
    units, out = build(draft, spans)
    recs = ec.records(draft, units)
    assert ec.apply(recs, draft) == out, (draft, spans, recs)
    prev_end = 0
    for pos, ref, alt, info in recs:
        assert pos - 1 >= prev_end and ref and alt
        prev_end = pos - 1 + len(ref)
        assert draft[pos - 1:pos - 1 + len(ref)] == ref
    return recs


def test_records_roundtrip_random():
    rnd = random.Random(11)
    for _ in range(400):
        draft = rand_seq(rnd, rnd.randint(1, 60))
        cuts = sorted(rnd.sample(range(len(draft) + 1), k=min(len(draft) + 1, 2 * rnd.randint(0, 4))))
        spans = []
        for b, e in zip(cuts[::2], cuts[1::2]):
            spans.append((b, e, mutate(rnd, draft[b:e], rnd.randint(0, 4)) if rnd.random() < 0.9 else ""))
        roundtrip(draft, spans)


def test_records_edge_cases():
    # an edit at position 0 (insertion, deletion, substitution)
    assert roundtrip("ACGTACGT", [(0, 3, "TACG")]) == [(1, "A", "TA", ".")]
    assert roundtrip("ACGTACGT", [(0, 3, "CG")]) == [(1, "AC", "C", ".")]
    assert roundtrip("ACGTACGT", [(0, 2, "GC")]) == [(1, "A", "G", ".")]
    # an insertion at the contig end
    assert roundtrip("ACGTACGT", [(6, 8, "GTAC")]) == [(8, "T", "TAC", ".")]
    assert roundtrip("ACGTACGT", [(6, 8, "GTTT")]) == [(7, "G", "GTT", ".")]
    # a whole contig emitted as nothing
    units, out = build("ACGTA", [(0, 5, "")])
    assert out == "" and ec.records("ACGTA", units) == [(1, "A", "<DEL>", "SVTYPE=DEL;END=5")]
    assert ec.apply(ec.records("ACGTA", units), "ACGTA") == ""
    # adjacent units (no draft text between them: one column stream)
    roundtrip("ACGTACGTAA", [(2, 4, "T"), (4, 6, "AAC")])
    # an insertion at 0, one matching base, an insertion: the two padded records share that base and are merged
    recs = roundtrip("ACGT", [(0, 1, "TAG")])
    assert recs == [(1, "A", "TAG", ".")]


def test_vcf_text_layout():
    txt = ec.vcf_text("d.fa", [("c1", 8, [(1, "A", "TA", ".")]), ("c2", 3, [])])
    lines = txt.splitlines()
    assert lines[0] == "##fileformat=VCFv4.2" and lines[2] == "##reference=d.fa"
    assert lines[3] == "##contig=<ID=c1,length=8>" and lines[-1] == "c1\t1\t.\tA\tTA\t.\tPASS\t."
