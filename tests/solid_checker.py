"""CPU checker of the solid k-mer construction (DESIGN.md "Solid k-mers from the reads"): an independent numpy restatement of
the whole contract, from the read files to the 4^k-bit set.  It shares no code with the host library or the kernels.

  parse_records(paths)     sequence of every record: FASTA (single- or multi-line) or FASTQ, plain or gzip, or "@list"
  count_canonical(seqs, k) canonical k-mers (min(fwd, rc), A0 C1 G2 T3, MSB-first) and their counts; ACGTacgt are bases, any
                           other byte ends a run, no k-mer spans two records
  histogram(counts, c)     hist[0 .. 4c] after the KMC filters -ci2 -cx<4c> (a k-mer counted more than 4c times is dropped)
  find_cutoffs(hist)       suk::SolidKmers::find_cutoffs with its 32-bit integer widths; None where the reference is undefined
  solid_set(...)           bits fwd and rc of every kept canonical k-mer without a homopolymer at either end
"""
import gzip
import os
import struct

import numpy as np

M32 = 0xFFFFFFFF
_LUT = np.full(256, 4, dtype=np.uint8)
for _i, _ch in enumerate(b"ACGT"):
    _LUT[_ch] = _i
    _LUT[_ch | 0x20] = _i


def _open_lines(path):
    with open(path, "rb") as f:
        magic = f.read(2)
    data = gzip.open(path, "rb").read() if magic == b"\x1f\x8b" else open(path, "rb").read()
    lines = data.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    return [l[:-1] if l.endswith(b"\r") else l for l in lines]


def expand_paths(paths):
    out = []
    for p in ([paths] if isinstance(paths, (str, os.PathLike)) else paths):
        p = os.fspath(p)
        if p.startswith("@"):
            out += [l.strip() for l in open(p[1:]) if l.strip()]
        else:
            out.append(p)
    return out


def parse_records(paths):
    """the sequence (bytes) of every record of every file, in order"""
    seqs = []
    for path in expand_paths(paths):
        lines = _open_lines(path)
        i = 0
        while i < len(lines) and lines[i] == b"":
            i += 1
        if i == len(lines):
            continue
        if lines[i][:1] not in (b">", b"@"):
            raise ValueError(f"{path}: neither FASTA nor FASTQ")
        if lines[i][:1] == b">":
            cur = None
            for l in lines[i:]:
                if l.startswith(b">"):
                    if cur is not None:
                        seqs.append(b"".join(cur))
                    cur = []
                elif l:
                    cur.append(l)
            if cur is not None:
                seqs.append(b"".join(cur))
            continue
        while i < len(lines):
            if lines[i] == b"":
                i += 1
                continue
            if not lines[i].startswith(b"@"):
                raise ValueError(f"{path}: malformed FASTQ")
            i += 1
            s = []
            while i < len(lines) and not lines[i].startswith(b"+"):
                s.append(lines[i])
                i += 1
            seq = b"".join(s)
            seqs.append(seq)
            if i < len(lines):
                i += 1
                q = 0
                while i < len(lines) and q < len(seq):
                    q += len(lines[i])
                    i += 1
    return seqs


def revcomp_codes(codes, k):
    codes = np.asarray(codes, dtype=np.uint64)
    r = np.zeros_like(codes)
    x = codes.copy()
    for _ in range(k):
        r = (r << np.uint64(2)) | (np.uint64(3) - (x & np.uint64(3)))
        x >>= np.uint64(2)
    return r


def count_canonical(seqs, k):
    """(canonical codes u64 sorted, counts i64) of every k-mer of the records"""
    data = b"\n".join(seqs) if not isinstance(seqs, (bytes, bytearray)) else bytes(seqs)
    b = _LUT[np.frombuffer(data, dtype=np.uint8)]
    n = b.size - k + 1
    if n <= 0:
        return np.zeros(0, np.uint64), np.zeros(0, np.int64)
    bad = np.concatenate([[0], np.cumsum(b > 3)])
    ok = (bad[k:k + n] - bad[:n]) == 0
    c = np.minimum(b, 3).astype(np.uint64)
    fwd = np.zeros(n, dtype=np.uint64)
    rc = np.zeros(n, dtype=np.uint64)
    for j in range(k):
        fwd = (fwd << np.uint64(2)) | c[j:j + n]
        rc |= (np.uint64(3) - c[j:j + n]) << np.uint64(2 * j)
    canon = np.minimum(fwd, rc)[ok]
    codes, counts = np.unique(canon, return_counts=True)
    return codes, counts.astype(np.int64)


def histogram(counts, coverage):
    top = 4 * coverage
    hist = np.zeros(top + 1, dtype=np.uint64)
    keep = (counts >= 2) & (counts <= top)
    np.add.at(hist, counts[keep], 1)
    return hist


def find_cutoffs(hist):
    """(err, mean, lower, upper) of suk::SolidKmers::find_cutoffs, or None when its mean would be unset"""
    h = [int(x) for x in hist]
    L = len(h) - 1
    ind = 2
    while ind < L and h[ind] > h[ind + 1]:
        ind += 1
    err_th = 2 if ind > 100 else ind
    gmv, mean = 0, None
    for ind in range(err_th + 1, L):
        if h[ind] > gmv:
            gmv = h[ind] & M32                       # UINT global_maxima_val = size_t
            mean = ind
    if mean is None:
        return None
    look = 5
    lower = err_th
    for ind in range(mean - 1, err_th - 1, -1):
        lo = ge = 0
        ind2 = ind - 1
        while ind2 >= ind - look and ind2 >= err_th:
            if h[ind2] < h[ind]:
                lo += 1
            else:
                ge += 1
            ind2 -= 1
        if ge >= lo:
            lower = ind
            break
    bind = mean + 1
    eind = min((bind + 2 * (mean - lower)) & M32, L)
    upper = eind
    plan_a = False
    for ind in range(bind, eind):
        lo = ge = 0
        for ind2 in range(ind + 1, min(ind + look, L - 1) + 1):
            if h[ind2] < h[ind]:
                lo += 1
            else:
                ge += 1
        if ge >= lo:
            upper, plan_a = ind, True
            break
    if not plan_a and bind < eind:
        delta = [0] * eind
        for ind in range(bind, eind):
            ds = lo = 0
            for ind2 in range(ind + 1, min(ind + look, L - 1) + 1):
                if h[ind2] < h[ind]:
                    lo += 1
                    ds = (ds + (h[ind] - h[ind2])) & M32
            delta[ind] = ((((ds * 100) & M32) // ((lo * h[ind]) & 0xFFFFFFFFFFFFFFFF)) & M32)
        best = np.float32(delta[bind])
        for ind in range(bind, eind):
            wl = min(look, eind - ind)
            s = sum(delta[ind:ind + wl]) & M32
            v = np.float32(np.float32(s) / np.float32(wl))
            if v < best:
                best, upper = v, ind
    return (err_th, mean, lower, upper)


def solid_set(codes, counts, k, coverage, lower, upper, exclude_hp=True):
    """(words u64[4^k / 64], set bits, canonical solid k-mers)"""
    keep = (counts >= 2) & (counts <= 4 * coverage) & (counts >= lower) & (counts <= upper)
    c = codes[keep]
    if exclude_hp:
        hi, hi2 = np.uint64(2 * (k - 1)), np.uint64(2 * (k - 2))
        three = np.uint64(3)
        ok = (((c >> hi) & three) != ((c >> hi2) & three)) & ((c & three) != ((c >> np.uint64(2)) & three))
        c = c[ok]
    words = np.zeros(max(1, (1 << (2 * k)) // 64), dtype=np.uint64)
    for x in (c, revcomp_codes(c, k)):
        np.bitwise_or.at(words, x >> np.uint64(6), np.uint64(1) << (x & np.uint64(63)))
    # distinct positions: a canonical code and its reverse complement, once for a palindrome (two kept codes never share one)
    n_bits = int(c.size) + int(np.count_nonzero(revcomp_codes(c, k) != c))
    return words, n_bits, int(c.size)


def build(paths_or_seqs, k, coverage):
    """the whole contract: dict(hist, cut, words, n_bits, n_canonical); cut None (and no set) where the reference is undefined"""
    if isinstance(paths_or_seqs, (bytes, bytearray)):
        seqs = [bytes(paths_or_seqs)]
    elif isinstance(paths_or_seqs, (list, tuple)) and paths_or_seqs and isinstance(paths_or_seqs[0], (bytes, bytearray)):
        seqs = list(paths_or_seqs)
    else:
        seqs = parse_records(paths_or_seqs)
    codes, counts = count_canonical(seqs, k)
    hist = histogram(counts, coverage)
    cut = find_cutoffs(hist)
    out = {"hist": hist, "cut": cut, "codes": codes, "counts": counts}
    if cut is not None:
        out["words"], out["n_bits"], out["n_canonical"] = solid_set(codes, counts, k, coverage, cut[2], cut[3])
    return out


def bvsd_bytes(words, k):
    """aux/solid_kmers.bvsd: sdsl bit_vector layout (uint64 bit count, then the words)"""
    return struct.pack("<Q", 1 << (2 * k)) + np.asarray(words, dtype="<u8").tobytes()


def cutoffs_line(cut):
    err, mean, lower, upper = cut
    return (f"[SolidKmers] Info: Error-threshold freq: {err}, Lower-threshold freq: {lower}, Upper-threshold freq: {upper}, "
            f"Mean-coverage: {mean}")
