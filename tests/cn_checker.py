"""CPU checker of `hypo --qv-cn` and of hypo_gpu_kset_query_depth (DESIGN.md "k-mer copy number"): the whole contract in plain
Python over two dicts, canonical k-mer -> how often the reads contain it and -> how often the text contains it, both stopping at
255.  It shares no code with the host library or the kernels.

  windows(seq, k)                   [(start, canonical code)] of every length-k window of `seq` made of ACGTacgt only (min(fwd, rc),
                                    A0 C1 G2 T3, MSB-first)
  tally(seqs, k)                    {code: min(255, windows of all seqs that have it)}; no window spans two of them
  depth(seqs, k, bin, reads, text, unit, t=1)
                                    the six arrays of hypo_gpu_kset_query_depth, bins numbered sequence by sequence: sequence s has
                                    ceil(len / bin) bins, bin j owns the windows that START in [j bin, (j + 1) bin).  With c = the
                                    window's read count and m = its text count: windows; missing (c < t, or not among the reads);
                                    rated (present, 1 <= m <= 254, c <= 254); over (rated, 2 c >= 3 unit m); under (rated,
                                    4 c <= 3 unit m); med_count (the lower median of c over the present windows, 0 without one)
  valley(h) / peak(h)               of a read histogram h[0 .. 256): the smallest c in 2..254 with h[c] <= h[c + 1] (2 without one);
                                    the c in [valley, 254] with the largest h[c], the smallest among equals, 0 when all are 0
  call(rated, over, under)          "collapsed" when 2 over > rated, "duplicated" when 2 under > rated, "." otherwise
  report(...) / parse_report        the file `hypo --qv-cn` writes, and back
  info_line(path, text)             the line `hypo` prints on stdout for it
"""
CAP = 255
HEADER = "#contig\tstart\tend\twindows\tmissing\trated\tover\tunder\tmedian_count\tcall"
_CODE = {ord(ch): i for i, ch in enumerate("ACGT")}
_CODE.update({ord(ch): i for i, ch in enumerate("acgt")})


def _bytes(seq):
    return seq.encode() if isinstance(seq, str) else bytes(seq)


def windows(seq, k):
    out, fwd, rc, run = [], 0, 0, 0
    mask, top = (1 << (2 * k)) - 1, 2 * (k - 1)
    for p, byte in enumerate(_bytes(seq)):
        c = _CODE.get(byte)
        if c is None:
            run = 0
            continue
        fwd = ((fwd << 2) | c) & mask
        rc = (rc >> 2) | ((3 - c) << top)
        run += 1
        if run >= k:
            out.append((p - k + 1, min(fwd, rc)))
    return out


def tally(seqs, k):
    d = {}
    for s in seqs:
        for _, code in windows(s, k):
            d[code] = d.get(code, 0) + 1
    return {code: min(n, CAP) for code, n in d.items()}


def n_bins(length, bin):
    return -(-length // bin)


def depth(seqs, k, bin, reads, text, unit, t=1):
    cols = {name: [] for name in ("windows", "missing", "rated", "over", "under", "med_count")}
    for s in seqs:
        s = _bytes(s)
        per_bin = [[] for _ in range(n_bins(len(s), bin))]
        for start, code in windows(s, k):
            per_bin[start // bin].append(code)
        for codes in per_bin:
            present = [(reads[c], text.get(c, 0)) for c in codes if reads.get(c, 0) >= t]
            rated = [(c, m) for c, m in present if 1 <= m <= 254 and c <= 254]
            cs = sorted(c for c, _ in present)
            cols["windows"].append(len(codes))
            cols["missing"].append(len(codes) - len(present))
            cols["rated"].append(len(rated))
            cols["over"].append(sum(1 for c, m in rated if 2 * c >= 3 * unit * m))
            cols["under"].append(sum(1 for c, m in rated if 4 * c <= 3 * unit * m))
            cols["med_count"].append(cs[(len(cs) + 1) // 2 - 1] if cs else 0)
    return cols


def histogram(reads):
    h = [0] * (CAP + 1)
    for n in reads.values():
        h[n] += 1
    return h


def valley(h):
    for c in range(2, CAP):
        if h[c] <= h[c + 1]:
            return c
    return 2


def peak(h):
    best = 0
    for c in range(valley(h), CAP):
        if h[c] > (h[best] if best else 0):
            best = c
    return best


def call(rated, over, under):
    return "collapsed" if 2 * over > rated else "duplicated" if 2 * under > rated else "."


def report(names, seqs, k, bin, reads, text, unit=None, t=1):
    """the file: unit None = the peak of the read histogram (ValueError when it has none)"""
    how = "peak" if unit is None else "given"
    if unit is None:
        unit = peak(histogram(reads))
        if not unit:
            raise ValueError("the read histogram has no peak")
    d = depth(seqs, k, bin, reads, text, unit, t)
    lines = [f"##hypo-qv-cn\tk={k}\tbin={bin}\tunit={unit}\t{how}\tmin_count={t}", HEADER]
    b = 0
    for name, s in zip(names, seqs):
        for j in range(n_bins(len(s), bin)):
            row = [d[c][b] for c in ("windows", "missing", "rated", "over", "under", "med_count")]
            lines.append("\t".join([name, str(j * bin), str(min((j + 1) * bin, len(s)))] + [str(x) for x in row] + [call(row[2], row[3], row[4])]))
            b += 1
    return "\n".join(lines) + "\n"


def parse_report(text):
    """{k, bin, unit, how, min_count, rows: [(contig, start, end, windows, missing, rated, over, under, median_count, call)]}"""
    lines = text.split("\n")
    assert lines[-1] == "" and lines[1] == HEADER, lines[:2]
    head = lines[0].split("\t")
    assert head[0] == "##hypo-qv-cn" and len(head) == 6 and head[4] in ("given", "peak"), lines[0]
    kv = dict(f.split("=") for f in head[1:4] + head[5:])
    out = {"k": int(kv["k"]), "bin": int(kv["bin"]), "unit": int(kv["unit"]), "how": head[4], "min_count": int(kv["min_count"]), "rows": []}
    for l in lines[2:-1]:
        f = l.split("\t")
        assert len(f) == 10 and f[9] in (".", "collapsed", "duplicated"), l
        out["rows"].append((f[0],) + tuple(int(x) for x in f[1:9]) + (f[9],))
    return out


def info_line(path, text):
    r = parse_report(text)
    n = {c: sum(1 for row in r["rows"] if row[9] == c) for c in ("collapsed", "duplicated")}
    bases = {c: sum(row[2] - row[1] for row in r["rows"] if row[9] == c) for c in ("collapsed", "duplicated")}
    return (f"[Hypo::Hypo] Info: copy number {path} (k = {r['k']}, bin = {r['bin']}, unit = {r['unit']} {r['how']}): {len(r['rows'])} bins, "
            f"{n['collapsed']} collapsed ({bases['collapsed']} bases), {n['duplicated']} duplicated ({bases['duplicated']} bases)")
