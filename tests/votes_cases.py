"""The inputs of the direct tests of the support votes (tests/test_votes_checker_cpu.py on the host loops,
tests/test_gpu_votes_direct.py on the kernels of support_kernel.hip): tables and reads as flat arrays, built by hand so that they
reach what generated genomes do not — repeats, the ends of the LDS tiles of both block shapes, gaps, 16-bit spans — and, for
every case, the condition that makes it worth running, computed from the inputs and the checker alone.

A case is built once per process, and so is what tests/votes_checker.py says about it (kmer_expected / min_expected)."""
import functools
from collections import namedtuple

import numpy as np

import votes_checker as vc

Reads = namedtuple("Reads", "rb re qae seq_off reads2")                      # the arrays of HypoArmsReads the votes read
KmerCase = namedtuple("KmerCase", "name k total_len spos kids reads")
MinCase = namedtuple("MinCase", "name total_len tables reads read_contig")

# what support_kernel.hip / capi.hip fix (the conditions below are stated in these terms)
KCAP = 2048                # solid k-mers of a 256-lane block's tile; a 64-lane block's holds KCAP / 4
MCAP = 1024                # minimizers likewise
LONG_SPAN = 1000           # mean reference span above which a block takes 64 reads instead of 256


# ---- building blocks -------------------------------------------------------------------------------------------------------------

def rand_codes(rng, n):
    return rng.integers(0, 4, size=n, dtype=np.uint8)


def periodic(unit, n):
    u = np.array(unit, dtype=np.uint8)
    return np.tile(u, n // u.size + 1)[:n]


def kmer_ids(codes, k):
    """the k-mer that starts at every position 0 .. n - k, as the scan stores it (first base in the top bits)"""
    mask = (1 << (2 * k)) - 1
    out, v = [], 0
    for i, b in enumerate(codes.tolist()):
        v = ((v << 2) | b) & mask
        if i + 1 >= k:
            out.append(v)
    return np.array(out, dtype=np.uint64)


def all_solid(codes, k):
    ids = kmer_ids(codes, k)
    return np.arange(ids.size, dtype=np.uint32), ids


def query_of(codes, rb, span, rng=None, n_edits=0):
    """the aligned query of a read over [rb, rb + span): a copy, with n_edits single-base insertions / deletions inside"""
    q = codes[rb:rb + span].tolist()
    for _ in range(n_edits):
        at = int(rng.integers(3, len(q) - 3))
        if rng.integers(0, 2):
            q.insert(at, int(rng.integers(0, 4)))
        else:
            del q[at]
    return q


def pack_reads(recs, odd_offsets=False):
    """recs: [(rb, span, query bases)] -> Reads sorted by rb, every read packed four bases to a byte from its own byte offset.
    odd_offsets: a spare byte goes in front of a read whenever its offset would be even.  Four spare bytes end the array: the
    kernels load the reads a 32-bit word at a time."""
    recs = sorted(recs, key=lambda r: r[0])
    rb = np.array([r[0] for r in recs], dtype=np.uint32)
    re = np.array([r[0] + r[1] for r in recs], dtype=np.uint32)
    qae = np.array([len(r[2]) for r in recs], dtype=np.uint32)
    seq_off = np.zeros(len(recs), dtype=np.uint64)
    chunks, at = [], 0
    for i, (_, _, q) in enumerate(recs):
        if odd_offsets and at % 2 == 0:
            chunks.append(np.full(1, 0xA5, dtype=np.uint8)); at += 1
        c = np.concatenate([np.array(q, dtype=np.uint8), np.zeros((-len(q)) % 4, np.uint8)]).reshape(-1, 4)
        chunks.append(((c[:, 0] << 6) | (c[:, 1] << 4) | (c[:, 2] << 2) | c[:, 3]).astype(np.uint8))
        seq_off[i] = at
        at += c.shape[0]
    chunks.append(np.zeros(4, dtype=np.uint8))
    return Reads(rb, re, qae, seq_off, np.concatenate(chunks))


def mean_span(reads):
    return int((reads.re.astype(np.int64) - reads.rb).sum()) // int(reads.rb.size)      # support_reads_of: integer mean


def lanes_of(reads):
    return 64 if mean_span(reads) > LONG_SPAN else 256


def read_spans(case):
    """[first, last) of every read of a k-mer case (tests/votes_checker.py: solid_span)"""
    sp = case.spos.tolist()
    return [vc.solid_span(sp, case.k, int(b), int(e)) for b, e in zip(case.reads.rb, case.reads.re)]


def kmer_blocks(case, lanes=None):
    """per block of `lanes` reads: (lowest first, highest last) over its reads that cover a solid k-mer, None when none does"""
    lanes = lanes or lanes_of(case.reads)
    spans = read_spans(case)
    out = []
    for b0 in range(0, len(spans), lanes):
        act = [(f, l) for f, l in spans[b0:b0 + lanes] if l > f]
        out.append((min(f for f, _ in act), max(l for _, l in act)) if act else None)
    return out


# ---- k-mer cases -----------------------------------------------------------------------------------------------------------------

def _repeats(k):
    rng = np.random.default_rng(100 + k)
    codes = np.concatenate([rand_codes(rng, 100), periodic([0], 200), rand_codes(rng, 100), periodic([0, 1, 2], 210), rand_codes(rng, 100),
                            periodic([3, 0, 2, 2, 1, 0, 3], 210), rand_codes(rng, 100)])
    n = codes.size
    spos, kids = all_solid(codes, k)
    recs = []
    for i, b in enumerate(range(0, n - 107, 15)):
        recs.append((b, 100, query_of(codes, b, 100)))                                   # an exact copy
        recs.append((b + 7, 100, query_of(codes, b + 7, 100, rng, 1 + i % 2)))            # one or two bases inserted or deleted
    return KmerCase(f"repeats_k{k}", k, n, spos, kids, pack_reads(recs))


def _repeats_cond(case, cov, sup, diag):
    assert diag["multi"] > 100 and diag["refused"] > 100, diag
    assert (case.reads.qae != case.reads.re - case.reads.rb).any()


def _range_ends():
    """reads with exactly k bases inserted or deleted in the middle: behind the edit every k-mer of the read lies k in front of or
    behind its place in the contig, on the very ends of [left, right]"""
    rng = np.random.default_rng(15)
    k = 11
    codes = rand_codes(rng, 1500)
    spos, kids = all_solid(codes, k)
    recs = []
    for i, b in enumerate(range(0, codes.size - 150, 33)):
        q = query_of(codes, b, 150)
        at = 60 + i % 20
        q = q[:at] + (rng.integers(0, 4, size=k).tolist() + q[at:] if i % 2 else q[at + k:])
        recs.append((b, 150, q))
    return KmerCase("range_ends", k, codes.size, spos, kids, pack_reads(recs))


def _range_ends_cond(case, cov, sup, diag):
    assert diag["at_left"] > 500 and diag["at_right"] > 500, diag


def _tags(kind):
    rng = np.random.default_rng({"low_byte": 21, "twice": 22, "borrow": 23, "high_bits": 24}[kind])
    if kind == "low_byte":
        # ACGT every eight bases, random between: every id gets ACGT's byte as its low byte, so the byte screen passes every
        # candidate and the whole id decides (the id is the contig's own k-mer where the contig has ACGT there)
        k = 13
        codes = rand_codes(rng, 1600)
        for p in range(0, codes.size - 4, 8):
            codes[p:p + 4] = [0, 1, 2, 3]
        spos, kids = all_solid(codes, k)
        kids = (kids & ~np.uint64(0xFF)) | np.uint64(0x1B)
    elif kind == "twice":
        k = 11
        codes = periodic([0, 1], 1200)
        spos, kids = all_solid(codes, k)
    elif kind == "borrow":
        # low bytes 0x00 and 0x01 next to each other: the zero-byte test flags a 0x01 above a 0x00 (a borrow), the whole id refuses it
        k = 9
        codes = np.concatenate([periodic([0, 0, 0, 0, 1], 600), rand_codes(rng, 100), periodic([0, 0, 0, 0, 0, 0, 1], 500)])
        spos, kids = all_solid(codes, k)
    else:
        # k = 17: the low 32 bits of an id are its last 16 bases.  A run of period d whose base in front breaks the period gives two
        # k-mers d apart that differ in the first base only
        k = 17
        parts = []
        for j in range(40):
            d = 1 + j % 4
            run = periodic(rng.permutation(4)[:d].tolist(), 16 + d + 6)
            # the k-mer at the base in front of the run and the one d behind it end in the same 16 bases (the run has period d);
            # they differ in their first base when the base in front is not run[d - 1]
            front = (int(run[d - 1]) + 1 + j % 3) % 4
            parts += [rand_codes(rng, 30), np.array([front], dtype=np.uint8), run]
        codes = np.concatenate(parts + [rand_codes(rng, 30)])
        spos, kids = all_solid(codes, k)
    n = codes.size
    recs = []
    for i, b in enumerate(range(0, n - 120, 11)):
        recs.append((b, 120, query_of(codes, b, 120, rng, (i % 3 == 2) * (1 + i % 2))))
    return KmerCase(f"tags_{kind}", k, n, spos, kids, pack_reads(recs))


def _tags_cond(case, cov, sup, diag):
    low = (case.kids & np.uint64(0xFF)).astype(np.int64)
    if case.name == "tags_low_byte":
        assert (low == low[0]).all()
        assert sup.sum() > 1000                           # (the true ids among them are found)
    elif case.name == "tags_twice":
        # whatever four consecutive entries a tag word holds, every byte in it is there at least twice
        for i in range(low.size - 3):
            w = low[i:i + 4].tolist()
            assert all(w.count(x) >= 2 for x in w)
    elif case.name == "tags_borrow":
        assert ((low[:-1] == 0) & (low[1:] == 1)).sum() > 100
    else:
        lo32 = (case.kids & np.uint64(0xFFFFFFFF)).astype(np.int64)
        pairs = sum(1 for i in range(lo32.size) for j in range(i + 1, min(i + case.k + 1, lo32.size))
                    if lo32[i] == lo32[j] and case.kids[i] != case.kids[j])
        assert pairs >= 40, pairs
        r = case.reads
        _, sup32 = vc.kmer_votes(case.k, case.spos, case.kids, r.rb, r.re, r.qae, r.seq_off, r.reads2, id_bits=32)
        assert (sup32 != sup).sum() > 20                  # a comparison of the low 32 bits votes differently


def _tiles256():
    rng = np.random.default_rng(31)
    k = 11
    n_reads = 600
    codes = rand_codes(rng, 20 * (n_reads - 1) + 150)
    spos, kids = all_solid(codes, k)
    recs = [(20 * i, 150, query_of(codes, 20 * i, 150, rng, (i % 10 == 3) * 2)) for i in range(n_reads)]
    return KmerCase("tiles256", k, codes.size + (codes.size & 1), spos, kids, pack_reads(recs))


def _tiles256_cond(case, cov, sup, diag):
    assert mean_span(case.reads) <= LONG_SPAN
    blocks = kmer_blocks(case, 256)
    assert len(blocks) == 3 and case.reads.rb.size % 256 != 0          # the last block is partly filled
    blo, bhi = blocks[0]
    assert bhi - blo > 2 * KCAP
    assert any(f < blo + KCAP < l for f, l in read_spans(case)[:256])   # a read's entries lie on both sides of the first tile's end


def _long_reads(extra_short):
    rng = np.random.default_rng(41)
    k = 13
    n_long, span = 68, 3000
    end_long = 100 * (n_long - 1) + span
    n_short = 160                                      # (68 * 3000 + 160 * 150) / 228 = 1000
    codes = rand_codes(rng, end_long + 30 * (n_short - 1) + 150)
    spos, kids = all_solid(codes, k)
    recs = [(100 * i, span, query_of(codes, 100 * i, span, rng, 3)) for i in range(n_long)]
    if extra_short:
        recs += [(end_long + 30 * j, 150, query_of(codes, end_long + 30 * j, 150)) for j in range(n_short)]
    return KmerCase("tiles64_plus_short" if extra_short else "tiles64", k, codes.size, spos, kids, pack_reads(recs))


def n_original_entries(case):
    """entries of the tiles64 tables that the appended short reads of tiles64_plus_short cannot touch: those in front of their start"""
    return int(np.searchsorted(case.spos, 100 * 67 + 3000))


def _tiles64_cond(case, cov, sup, diag):
    if case.name == "tiles64":
        assert mean_span(case.reads) > LONG_SPAN and lanes_of(case.reads) == 64
        assert all(l - f > 4 * (KCAP // 4) for f, l in read_spans(case))
        assert len(kmer_blocks(case, 64)) == 2
    else:
        assert mean_span(case.reads) == LONG_SPAN and lanes_of(case.reads) == 256
        blo, bhi = kmer_blocks(case, 256)[0]
        assert bhi - blo > 2 * KCAP


def _gaps():
    rng = np.random.default_rng(51)
    k = 11
    codes = rand_codes(rng, 10_400)
    spos, kids = all_solid(codes, k)
    recs = [(25 * i, 150, query_of(codes, 25 * i, 150)) for i in range(60)] + [(8600 + 25 * i, 150, query_of(codes, 8600 + 25 * i, 150)) for i in range(60)]
    return KmerCase("gaps", k, codes.size, spos, kids, pack_reads(recs))


def gap_range(case):
    spans = read_spans(case)
    return max(l for f, l in spans[:60]), min(f for f, l in spans[60:])


def _gaps_cond(case, cov, sup, diag):
    assert case.reads.rb.size <= 256 and lanes_of(case.reads) == 256       # one block
    g0, g1 = gap_range(case)
    assert g1 - g0 > 3 * KCAP
    assert not cov[g0:g1].any() and not sup[g0:g1].any()
    assert cov[:g0].any() and cov[g1:].any()


def _edges(k):
    rng = np.random.default_rng(600 + k)
    n = 400
    codes = rand_codes(rng, n)
    codes[300:340] = periodic([1, 2], 40)              # (some repeats for k = 2 and the reads at the end)
    spos, kids = all_solid(codes, k)
    keep = (spos < 250) | (spos >= 300)                # no solid k-mer starts in [250, 300)
    spos, kids = spos[keep], kids[keep]
    recs = [(0, 50, query_of(codes, 0, 50)),                                    # at coordinate 0
            (n - 60, 60, query_of(codes, n - 60, 60)),                          # ends at total_len
            (100, 60, query_of(codes, 100, 60, rng, 1)),
            (200, max(k - 1, 1), query_of(codes, 200, max(k - 1, 1))),          # shorter than k
            (258, 34, query_of(codes, 258, 34))]                                # over no solid k-mer
    recs += [(110 + 3 * j, 40 + j, query_of(codes, 110 + 3 * j, 40 + j)) for j in range(16)]      # qae of every residue mod 16
    return KmerCase(f"edges_k{k}", k, n, spos, kids, pack_reads(recs, odd_offsets=True))


def _edges_cond(case, cov, sup, diag):
    r, k, sp = case.reads, case.k, set(case.spos.tolist())
    assert (r.rb == 0).any() and (r.re == case.total_len).any()
    assert any(int(e) - k in sp and int(e) + 1 - k in sp for e in r.re)          # spos + k == re and spos + k == re + 1
    assert (r.re - r.rb < k).any()
    assert any(f == l for f, l in read_spans(case))
    assert set((r.qae % 16).tolist()) == set(range(16))
    assert (r.seq_off % 2 == 1).all()
    assert sup.sum() > 0


KMER_CASES = {
    "repeats_k5": (lambda: _repeats(5), _repeats_cond), "repeats_k11": (lambda: _repeats(11), _repeats_cond),
    "tags_low_byte": (lambda: _tags("low_byte"), _tags_cond), "tags_twice": (lambda: _tags("twice"), _tags_cond),
    "tags_borrow": (lambda: _tags("borrow"), _tags_cond), "tags_high_bits": (lambda: _tags("high_bits"), _tags_cond),
    "range_ends": (_range_ends, _range_ends_cond),
    "tiles256": (_tiles256, _tiles256_cond),
    "tiles64": (lambda: _long_reads(False), _tiles64_cond), "tiles64_plus_short": (lambda: _long_reads(True), _tiles64_cond),
    "gaps": (_gaps, _gaps_cond),
}
KMER_CASES.update({f"edges_k{k}": (functools.partial(_edges, k), _edges_cond) for k in (2, 15, 16, 17, 31)})


@functools.lru_cache(maxsize=None)
def kmer_case(name):
    return KMER_CASES[name][0]()


@functools.lru_cache(maxsize=None)
def kmer_expected(name):
    """(coverage, support, diagnostics) of the checker"""
    c = kmer_case(name)
    diag = {}
    cov, sup = vc.kmer_votes(c.k, c.spos, c.kids, c.reads.rb, c.reads.re, c.reads.qae, c.reads.seq_off, c.reads.reads2, diag=diag)
    cov.setflags(write=False); sup.setflags(write=False)
    return cov, sup, diag


def kmer_condition(name):
    KMER_CASES[name][1](kmer_case(name), *kmer_expected(name))


# the narrow-id kernel: a contig for hypo_gpu_solid_scan_keep (every 9-mer solid) and reads that make its blocks cross tiles; the
# tables are what the scan reports, so the test builds the KmerCase itself
def kept_contig_and_reads():
    rng = np.random.default_rng(71)
    parts = []
    while sum(p.size for p in parts) < 20_000:
        j = len(parts)
        parts.append([rand_codes(rng, 400), periodic([j % 4], 150), periodic([0, 3, 1], 200), periodic([2, 2, 1, 0, 3, 1, 1], 200),
                      np.tile(rand_codes(rng, 50), 6)][j % 5])
    codes = np.concatenate(parts)[:20_000]
    recs = [(20 * i, 150, query_of(codes, 20 * i, 150, rng, (i % 7 == 1) * 1)) for i in range((codes.size - 150) // 20)]
    return codes, pack_reads(recs)


# ---- minimizer cases -------------------------------------------------------------------------------------------------------------

def contig_minimizers(codes, beg, end):
    """[(position, k-mer)] of the window minimizers of codes[beg:end], positions in the contig"""
    return [(beg + s, key) for key, s in vc.read_minimizers(codes[beg:end].tolist())]


def every_position(codes, beg, end):
    ids = kmer_ids(codes[beg:end], vc.MIN_K)
    return [(beg + 1 + i, int(ids[1 + i])) for i in range(ids.size - 1)]      # from beg + 1 on: every rel_pos is 1


def mega_tables(contigs):
    """contigs: [(borders, even, {window index: [(position, k-mer)]})] -> (MegaTables, total_len).  A contig gets one
    MWMinimiserInfo per mega-window index a read can name ((borders - 1) / 2 + 1 of them, the last may be a window of no bases, as
    after Contig::prepare_for_division) and starts at an even coordinate."""
    contig_base, reg_base, win_even, info_base, start, mw_off, rel_pos, mins = [], [0], [], [], [], [0], [], []
    base = n_info = 0
    for borders, even, entries in contigs:
        contig_base.append(base); win_even.append(1 if even else 0); info_base.append(n_info)
        start += list(borders)
        reg_base.append(len(start))
        for x in range((len(borders) - 1) // 2 + 1):
            w = 2 * x if even else 2 * x + 1
            ent = entries.get(w, [])
            assert not ent or (w + 1 < len(borders) and borders[w] <= ent[0][0] and ent[-1][0] < borders[w + 1])
            at = borders[w] if ent else 0
            for p, key in ent:
                rel_pos.append(p - at); mins.append(key); at = p
            mw_off.append(len(rel_pos))
            n_info += 1
        base += borders[-1] + (borders[-1] & 1)
    u32 = lambda a: np.array(a, dtype=np.uint32)
    return vc.MegaTables(u32(contig_base), u32(reg_base), np.array(win_even, dtype=np.uint8), u32(info_base), u32(start), n_info, u32(mw_off), u32(rel_pos), u32(mins)), base


def entry_positions(T):
    """contig-local position and contig of every entry of the tables"""
    pos = np.zeros(int(T.mw_off[T.n_info]), dtype=np.int64)
    ctg = np.zeros(pos.size, dtype=np.int64)
    for c in range(T.contig_base.size):
        x1 = int(T.info_base[c + 1]) if c + 1 < T.info_base.size else T.n_info
        for x in range(int(T.info_base[c]), x1):
            xl = x - int(T.info_base[c])
            w = 2 * xl if T.win_even[c] else 2 * xl + 1
            e0, e1 = int(T.mw_off[x]), int(T.mw_off[x + 1])
            if e0 < e1:
                pos[e0:e1] = int(T.start[int(T.reg_base[c]) + w]) + np.cumsum(T.rel_pos[e0:e1].astype(np.int64))
                ctg[e0:e1] = c
    return pos, ctg


def min_blocks(case, lanes=None):
    """per block: (lowest first entry, end of the last mega-window) over its reads that cover an entry — the stretch of the tables
    a block of support_minimizers_kernel walks; None when no read of it covers one"""
    T, r = case.tables, case.reads
    lanes = lanes or lanes_of(r)
    pos, _ = entry_positions(T)
    per_read = []
    for a in range(r.rb.size):
        c = int(case.read_contig[a])
        b, e = int(r.rb[a]) - int(T.contig_base[c]), int(r.re[a]) - int(T.contig_base[c])
        fw, lw = vc.mega_windows_of(T, c, b, e)
        if lw < fw:
            per_read.append(None); continue
        even = bool(T.win_even[c])
        x0 = int(T.info_base[c]) + (fw // 2 if even else (fw - 1) // 2)
        x1 = int(T.info_base[c]) + (lw // 2 if even else (lw - 1) // 2)
        lo, hi = int(T.mw_off[x0]), int(T.mw_off[x0 + 1])
        e0 = lo + int(np.searchsorted(pos[lo:hi], b))
        e1 = int(T.mw_off[x1 + 1])
        covered = e0 < e1 and pos[e0] < e
        per_read.append((e0, e1) if covered else None)
    out = []
    for b0 in range(0, len(per_read), lanes):
        act = [x for x in per_read[b0:b0 + lanes] if x]
        out.append((min(x[0] for x in act), max(x[1] for x in act)) if act else None)
    return out


def _min_reads(contigs_codes, T, specs, rng):
    """specs: [(contig, rb, span, n_edits)], contig-local -> (Reads, read_contig), sorted by coordinate"""
    specs = sorted(specs, key=lambda s: (s[0], s[1]))
    recs = [(int(T.contig_base[c]) + b, s, query_of(contigs_codes[c], b, s, rng, ne)) for c, b, s, ne in specs]
    return pack_reads(recs), np.array([s[0] for s in specs], dtype=np.uint32)


GEO_BORDERS = ([0, 600, 700, 1500, 1560, 2400, 2500, 3001], [0, 900, 1000, 2000], [0, 80, 900, 1000, 1800, 1850, 2601], [0, 500, 560, 1200])


def _geometry_tables():
    rng = np.random.default_rng(81)
    codes = [rand_codes(rng, b[-1]) for b in GEO_BORDERS]
    full = lambda c, borders, ws: {w: contig_minimizers(codes[c], borders[w], borders[w + 1]) for w in ws}
    contigs = [(GEO_BORDERS[0], True, full(0, GEO_BORDERS[0], (0, 2, 4, 6))), (GEO_BORDERS[1], True, full(1, GEO_BORDERS[1], (0, 2))),
               (GEO_BORDERS[2], False, full(2, GEO_BORDERS[2], (1, 3, 5))), (GEO_BORDERS[3], True, {})]
    T, total = mega_tables(contigs)
    return codes, T, total


def _geometry(indels):
    codes, T, total = _geometry_tables()
    rng = np.random.default_rng(82 + indels)
    pos, ctg = entry_positions(T)
    specs = []
    for c in (0, 2, 3):
        n = GEO_BORDERS[c][-1]
        specs += [(c, b, 150, (i % 2 + 1) if indels else 0) for i, b in enumerate(range(0, n - 150, 37))]
        specs.append((c, n - 150, 150, 0))                                   # ends in the last region, at the contig's end
    if not indels:
        specs += [(0, 700, 150, 0), (0, 600, 150, 0), (2, 900, 120, 0),      # start exactly on a border
                  (0, 610, 80, 0), (2, 10, 60, 0), (2, 1805, 40, 0),         # wholly inside an SR region
                  (0, 500, 1200, 0), (2, 40, 2000, 0),                       # span several mega-windows
                  (0, 1300, 150, 0), (2, 700, 150, 0)]                       # start deep inside a long mega-window
        for c in (0, 2):                                                     # minimizers at exactly rb, re - 1 and re
            p = int(pos[ctg == c][len(pos[ctg == c]) // 2])
            specs += [(c, p, 150, 0), (c, p + 1 - 150, 150, 0), (c, p - 150, 150, 0)]
    reads, read_contig = _min_reads(codes, T, specs, rng)
    return MinCase("indels" if indels else "geometry", total, T, reads, read_contig)


def _geometry_cond(case, cov, sup):
    T, r = case.tables, case.reads
    assert len(set(T.contig_base.tolist())) == 4 and set(T.win_even.tolist()) == {0, 1}
    assert 1 not in case.read_contig and 3 in case.read_contig
    pos, ctg = entry_positions(T)
    assert not (ctg == 3).any() and (ctg == 1).any() and not cov[ctg == 1].any()
    assert cov.sum() > 0 and sup.sum() > 0
    if case.name == "indels":
        assert (r.qae != r.re - r.rb).sum() > 100
        return
    seen = {"border": 0, "in_sr": 0, "several": 0, "last": 0, "at_rb": 0, "at_re_1": 0, "at_re": 0, "deep": 0}
    for a in range(r.rb.size):
        c = int(case.read_contig[a])
        b, e = int(r.rb[a]) - int(T.contig_base[c]), int(r.re[a]) - int(T.contig_base[c])
        borders = T.start[int(T.reg_base[c]):int(T.reg_base[c + 1])].tolist()
        reg_b = max(i for i, x in enumerate(borders) if x <= b)
        reg_e = max(i for i, x in enumerate(borders) if x < e)
        is_mw = lambda i: (i % 2 == 0) == bool(T.win_even[c])
        seen["border"] += b in borders and b > 0
        seen["in_sr"] += reg_b == reg_e and not is_mw(reg_b)
        seen["several"] += sum(1 for i in range(reg_b, reg_e + 1) if is_mw(i)) >= 2
        seen["last"] += e == borders[-1]
        seen["deep"] += is_mw(reg_b) and b - borders[reg_b] >= 500
        here = set(pos[ctg == c].tolist())
        seen["at_rb"] += b in here; seen["at_re_1"] += (e - 1) in here; seen["at_re"] += e in here
    assert all(v > 0 for v in seen.values()), seen


def _ties():
    rng = np.random.default_rng(91)
    codes = np.concatenate([rand_codes(rng, 200), periodic([0], 400), rand_codes(rng, 100), periodic([2, 1], 400), rand_codes(rng, 100), periodic([3], 300), rand_codes(rng, 101)])
    n = codes.size
    borders = [0, 150, 180, n]
    T, total = mega_tables([(borders, True, {0: contig_minimizers(codes, 0, 150), 2: contig_minimizers(codes, 180, n)})])
    specs = [(0, b, 150, (i % 4 == 3) * 1) for i, b in enumerate(range(0, n - 150, 13))]
    reads, read_contig = _min_reads([codes], T, specs, rng)
    return MinCase("ties", total, T, reads, read_contig)


def _ties_cond(case, cov, sup):
    T = case.tables
    pos, _ = entry_positions(T)
    m = T.minimisers.astype(np.int64)
    # the same minimizer several times within 50 bases
    assert sum(1 for i in range(m.size - 3) if m[i] == m[i + 3] and pos[i + 3] - pos[i] < 50) > 100
    # and reads whose windows hold equal keys: an entry supported more than once by one read shows in support > coverage
    assert (sup > cov).any()


def _min_tiles(long_reads):
    rng = np.random.default_rng(95)
    n = 3300
    codes = rand_codes(rng, n)
    codes[1000:1400] = periodic([0, 0, 1], 400)
    T, total = mega_tables([([0, n], True, {0: every_position(codes, 0, n)})])
    if long_reads:
        specs = [(0, 30 * i, 1200, i % 3) for i in range(70)]
    else:
        specs = [(0, 10 * i, 150, (i % 9 == 4) * 1) for i in range(300)]
    reads, read_contig = _min_reads([codes], T, specs, rng)
    return MinCase("tiles64" if long_reads else "tiles256", total, T, reads, read_contig)


def _min_tiles_cond(case, cov, sup):
    assert (case.tables.rel_pos == 1).all()
    lanes = lanes_of(case.reads)
    assert lanes == (64 if case.name == "tiles64" else 256)
    blocks = min_blocks(case)
    assert len(blocks) == 2
    blo, bhi = blocks[0]
    assert bhi - blo > (MCAP if lanes == 256 else MCAP // 4)
    assert sup.sum() > 0


def _sixteen_bits(with_short):
    rng = np.random.default_rng(97)
    n = 75_000
    codes = rand_codes(rng, n)
    borders = [0, 40_000, 40_050, n]
    T, total = mega_tables([(borders, True, {0: contig_minimizers(codes, 0, 40_000), 2: contig_minimizers(codes, 40_050, n)})])
    specs = [(0, 1000, 70_000, 0)] + [(0, 3500 * i, 3000, i % 2) for i in range(20)]
    if with_short:
        specs += [(0, 66_000 + 40 * i, 150, 0) for i in range(130)]
    reads, read_contig = _min_reads([codes], T, specs, rng)
    return MinCase("sixteen_bits_256" if with_short else "sixteen_bits_64", total, T, reads, read_contig)


def _sixteen_bits_cond(case, cov, sup):
    T, r = case.tables, case.reads
    assert lanes_of(r) == (256 if case.name.endswith("256") else 64)
    a = int(np.argmax(r.re - r.rb))
    assert int(r.re[a] - r.rb[a]) > 65_535
    pos, _ = entry_positions(T)
    assert ((pos >= int(r.rb[a]) + 65_506) & (pos < int(r.re[a]))).sum() > 100
    _, wide = vc.minimizer_votes(T, r.rb, r.re, r.qae, r.seq_off, r.reads2, case.read_contig, wide=True)
    assert (wide != sup).sum() > 100


MIN_CASES = {
    "geometry": (lambda: _geometry(0), _geometry_cond), "indels": (lambda: _geometry(1), _geometry_cond),
    "ties": (_ties, _ties_cond),
    "tiles256": (lambda: _min_tiles(False), _min_tiles_cond), "tiles64": (lambda: _min_tiles(True), _min_tiles_cond),
    "sixteen_bits_64": (lambda: _sixteen_bits(False), _sixteen_bits_cond), "sixteen_bits_256": (lambda: _sixteen_bits(True), _sixteen_bits_cond),
}


@functools.lru_cache(maxsize=None)
def min_case(name):
    return MIN_CASES[name][0]()


@functools.lru_cache(maxsize=None)
def min_expected(name):
    c = min_case(name)
    r = c.reads
    cov, sup = vc.minimizer_votes(c.tables, r.rb, r.re, r.qae, r.seq_off, r.reads2, c.read_contig)
    cov.setflags(write=False); sup.setflags(write=False)
    return cov, sup


def min_condition(name):
    MIN_CASES[name][1](min_case(name), *min_expected(name))
