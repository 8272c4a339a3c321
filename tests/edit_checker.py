"""Restatement of the `hypo --vcf` contract (DESIGN.md "Edit scripts") for the tests: the canonical unit-cost alignment as a
full numpy matrix, the record builder, the VCF writer, an applier, and the replacement units of a run rebuilt from its
HYPO_REGION_DUMP file."""
import numpy as np

OPS = "=XDI"


def align(a, b):
    """(distance, ops) of the canonical alignment of a (draft span) against b: ops is a string over '=XDI' in draft order.
    Row sweep: the diagonal and up terms are vectors, the left term a running minimum (np.minimum.accumulate of c[j] - j)."""
    a = np.frombuffer(bytes(a), dtype=np.uint8)
    b = np.frombuffer(bytes(b), dtype=np.uint8)
    n, m = a.size, b.size
    j = np.arange(m + 1, dtype=np.int64)
    move = np.zeros((n + 1, m + 1), dtype=np.uint8)      # 0 '=', 1 'X', 2 up ('D'), 3 left ('I')
    move[0, 1:] = 3
    move[1:, 0] = 2
    prev = j.copy()
    for i in range(1, n + 1):
        x = (b != a[i - 1]).astype(np.int64)
        diag = prev[:-1] + x
        up = prev[1:] + 1
        c = np.empty(m + 1, dtype=np.int64)
        c[0] = i
        c[1:] = np.minimum(diag, up)
        row = np.minimum.accumulate(c - j) + j
        mv = np.full(m + 1, 3, dtype=np.uint8)
        mv[1:][row[1:] == up] = 2
        is_diag = row[1:] == diag
        mv[1:][is_diag] = x[is_diag].astype(np.uint8)
        mv[0] = 2
        move[i] = mv
        prev = row
    ops = []
    i, jj = n, m
    while i or jj:
        o = move[i, jj]
        ops.append(OPS[o])
        if o < 2:
            i -= 1
            jj -= 1
        elif o == 2:
            i -= 1
        else:
            jj -= 1
    return int(prev[m]), "".join(reversed(ops))


def align_trimmed(a, b):
    """align() with the shortcuts the contract allows: the common suffix is trimmed (exact), a == b and empty sides need no DP"""
    a, b = bytes(a), bytes(b)
    if a == b:
        return 0, "=" * len(a)
    s = 0
    while s < min(len(a), len(b)) and a[len(a) - 1 - s] == b[len(b) - 1 - s]:
        s += 1
    a2, b2 = a[:len(a) - s], b[:len(b) - s]
    if not a2 or not b2:
        return len(a2) + len(b2), "D" * len(a2) + "I" * len(b2) + "=" * s
    d, ops = align(a2, b2)
    return d, ops + "=" * s


def runs(ops):
    out = []
    for o in ops:
        if out and out[-1][1] == o:
            out[-1][0] += 1
        else:
            out.append([1, o])
    return [(n, o) for n, o in out]


def cigar(ops):
    return "".join(f"{n}{o}" for n, o in runs(ops))


def parse_cigar(c):
    out, num = [], ""
    for ch in c:
        if ch.isdigit():
            num += ch
        else:
            out.append((int(num), ch))
            num = ""
    return out


def records(draft, units):
    """draft: str; units: [(beg, end, text, cigar_runs)] sorted and disjoint, cigar_runs = [(len, op)] aligning draft[beg:end]
    against text.  Returns [(pos1, ref, alt, info)]."""
    out_len = len(draft) - sum(e - b for b, e, _, _ in units) + sum(len(t) for _, _, t, _ in units)
    if draft and out_len == 0:
        return [(1, draft[0], "<DEL>", f"SVTYPE=DEL;END={len(draft)}")]
    raw, cur = [], None
    dp = 0

    def close():
        nonlocal cur
        if cur is not None:
            raw.append((cur[0], cur[1], "".join(cur[2])))
            cur = None
    for beg, end, text, rl in units:
        if beg > dp:
            close()
        dp, tp = beg, 0
        for ln, op in rl:
            if op == "=":
                if ln:
                    close()
                dp += ln
                tp += ln
                continue
            if cur is None:
                cur = [dp, dp, []]
            if op in "XI":
                cur[2].append(text[tp:tp + ln])
                tp += ln
            if op in "XD":
                dp += ln
            cur[1] = dp
        assert dp == end and tp == len(text), "unit script does not span its unit"
    close()
    recs = []
    for rb, re_, alt in raw:
        ref = draft[rb:re_]
        if not ref or not alt:
            if rb > 0:
                rb -= 1
                ref, alt = draft[rb] + ref, draft[rb] + alt
            else:
                ref, alt = ref + draft[re_], alt + draft[re_]
                re_ += 1
        if recs and recs[-1][1] > rb:        # a record at 0 padded with the base after, and one padded with that same base
            pb, pe, palt = recs.pop()
            alt = palt + alt[pe - rb:]
            rb = pb
        recs.append((rb, re_, alt))
    return [(rb + 1, draft[rb:re_], alt, ".") for rb, re_, alt in recs]


def read_fastx(path):
    """[(name, seq)] of a FASTA / FASTQ file, plain or gzip (name = the header up to the first white space)"""
    import gzip
    raw = open(path, "rb").read()
    if raw[:2] == b"\x1f\x8b":
        raw = gzip.decompress(raw)
    lines = raw.decode().splitlines()
    out, i = [], 0
    while i < len(lines):
        l = lines[i]
        if l.startswith(">"):
            name, seq = l[1:].split()[0] if l[1:].split() else "", []
            i += 1
            while i < len(lines) and not lines[i].startswith(">"):
                seq.append(lines[i].strip())
                i += 1
            out.append((name, "".join(seq)))
        elif l.startswith("@"):
            out.append((l[1:].split()[0], lines[i + 1].strip()))
            i += 4
        else:
            i += 1
    return out


def vcf_text(reference, contigs):
    """contigs: [(name, draft_len, records)] in draft order"""
    lines = ["##fileformat=VCFv4.2", "##source=hypo", f"##reference={reference}"]
    lines += [f"##contig=<ID={n},length={ln}>" for n, ln, _ in contigs]
    lines += ['##ALT=<ID=DEL,Description="Deletion">',
              '##INFO=<ID=SVTYPE,Number=1,Type=String,Description="Type of structural variant">',
              '##INFO=<ID=END,Number=1,Type=Integer,Description="End position of the variant">',
              "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"]
    for n, _, recs in contigs:
        lines += [f"{n}\t{p}\t.\t{r}\t{a}\t.\tPASS\t{i}" for p, r, a, i in recs]
    return "\n".join(lines) + "\n"


def apply(recs, draft):
    """draft with every record's REF replaced by its ALT (checks that REF matches and that records do not overlap)"""
    out, at = [], 0
    for pos, ref, alt, info in recs:
        b = pos - 1
        assert b >= at, "records overlap or are out of order"
        assert draft[b:b + len(ref)] == ref, f"REF {ref} does not match the draft at {pos}"
        out.append(draft[at:b])
        out.append("" if alt == "<DEL>" else alt)
        at = b + (len(draft) if alt == "<DEL>" else len(ref))
    out.append(draft[at:])
    return "".join(out)


def parse_vcf(text):
    """{contig: [(pos, ref, alt, info)]} and the header lines"""
    head, recs = [], {}
    for l in text.splitlines():
        if l.startswith("#"):
            head.append(l)
            continue
        f = l.split("\t")
        recs.setdefault(f[0], []).append((int(f[1]), f[3], f[4], f[7]))
    return head, recs


def units_from_dump(dump_path, names, drafts, long_reads):
    """{name: [(beg, end, text)]}: the replacement units of a run from its HYPO_REGION_DUMP file.  A line with text in column 10
    replaces [b, e); SR / MSR lines, and (short-only runs) lines of window-less regions, are draft text; draft positions no line
    covers are emitted as nothing.  Also returns {name: output text}."""
    rows = {}
    for l in open(dump_path):
        f = l.rstrip("\n").split("\t")
        rows.setdefault(f[0], []).append(f)
    units, outs = {}, {}
    for name in names:
        d = drafts[name]
        segs = []                                    # (beg, end, text, verbatim)
        for f in sorted(rows.get(name, []), key=lambda f: int(f[1])):
            b, e, t = int(f[1]), int(f[2]), f[3]
            if t in ("SR", "MSR"):
                segs.append((b, e, d[b:e], True))
            else:
                verb = not long_reads and all(x == "0" for x in f[4:9])
                segs.append((b, e, f[9], verb))
        us, out, cur, at = [], [], None, 0
        for b, e, text, verb in segs + [(len(d), len(d), "", True)]:
            assert b >= at, f"{name}: dump lines overlap at {b}"
            if verb:
                if cur is not None or b > at:
                    ub = cur[0] if cur is not None else at
                    us.append((ub, b, "".join(cur[1]) if cur is not None else ""))
                    cur = None
                out.append(text)
            else:
                if cur is None:
                    cur = [at, []]
                cur[1].append(text)
                out.append(text)
            at = e
        units[name] = [u for u in us if u[1] > u[0] or u[2]]
        outs[name] = "".join(out)
    return units, outs
