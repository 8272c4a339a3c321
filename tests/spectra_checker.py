"""CPU checker of `hypo --qv-spectra` (DESIGN.md "k-mer spectra"): the whole contract in plain Python / numpy, from the read
files to the file.  It shares no code with the host library or the kernels.

  read_counts(paths_or_seqs, k)   (keys, counts): the distinct canonical k-mers (min(fwd, rc), A0 C1 G2 T3, MSB-first) of all
                                  records as a sorted u64 array, and how many length-k windows of the records have each of them,
                                  stopping at 255.  The byte rules are those of qv_checker: ACGTacgt are bases, any other byte or a
                                  record end ends a run.  Every window counts once, a palindromic one too.
  copy_numbers(texts, k, keys)    (cn, asm_only): per read k-mer the windows of all `texts` (the contigs of a draft, or of the
                                  polished FASTA) that have it, stopping at 255, and the number of windows whose k-mer no read has
  spectrum(counts, cn)            S[c][j], c = 0..255, j = 0..4: the read k-mers with count == c and min(cn, 4) == j (i64[256, 5])
  valley(h)                       the reliable threshold: the smallest c in 2..254 with h[c] <= h[c + 1], 2 when there is none
  completeness(S, t)              (reliable, found, text): reliable = sum_{c >= t} h[c], found = those with cn >= 1; "%.6f" or "NA"
  report(...) / parse_report      the file `hypo --qv-spectra` writes, and back
"""
import numpy as np

import qv_checker as qc
import solid_checker as sc

CAP = 255
COLS = 5
COLUMNS = ("#multiplicity\tdraft_cn0\tdraft_cn1\tdraft_cn2\tdraft_cn3\tdraft_cn4+\t"
           "polished_cn0\tpolished_cn1\tpolished_cn2\tpolished_cn3\tpolished_cn4+")
TEXT_HEADER = "#text\treliable\tfound\tcompleteness\tasm_only_windows"


def _records(paths_or_seqs):
    if isinstance(paths_or_seqs, (bytes, bytearray)):
        return [bytes(paths_or_seqs)]
    if isinstance(paths_or_seqs, (list, tuple)) and (not paths_or_seqs or isinstance(paths_or_seqs[0], (bytes, bytearray))):
        return list(paths_or_seqs)
    return sc.parse_records(paths_or_seqs)


def _tally(seqs, k):
    """(sorted distinct canonical k-mers, unsaturated window counts) of byte strings; no window spans two of them"""
    keys, counts = np.zeros(0, np.uint64), np.zeros(0, np.int64)
    for i in range(0, len(seqs), 4096):
        u, c = np.unique(qc.canonical_windows(b"\n".join(seqs[i:i + 4096]), k), return_counts=True)
        allk = np.concatenate([keys, u])
        allc = np.concatenate([counts, c.astype(np.int64)])
        keys, inv = np.unique(allk, return_inverse=True)
        counts = np.bincount(inv, weights=allc, minlength=keys.size).astype(np.int64)
    return keys, counts


def read_counts(paths_or_seqs, k):
    keys, counts = _tally(_records(paths_or_seqs), k)
    return keys, np.minimum(counts, CAP)


def copy_numbers(texts, k, keys):
    texts = [t.encode() if isinstance(t, str) else bytes(t) for t in texts]
    tk, tc = _tally(texts, k)
    cn = np.zeros(keys.size, np.int64)
    if keys.size == 0 or tk.size == 0:
        return cn, int(tc.sum())
    at = np.minimum(np.searchsorted(keys, tk), keys.size - 1)
    hit = keys[at] == tk
    cn[at[hit]] = tc[hit]
    return np.minimum(cn, CAP), int(tc[~hit].sum())


def spectrum(counts, cn):
    S = np.zeros((CAP + 1, COLS), np.int64)
    np.add.at(S, (np.asarray(counts, np.int64), np.minimum(np.asarray(cn, np.int64), COLS - 1)), 1)
    return S


def histogram(S):
    return np.asarray(S).sum(axis=1)


def valley(h):
    for c in range(2, CAP):
        if h[c] <= h[c + 1]:
            return c
    return 2


def completeness(S, t):
    S = np.asarray(S)
    reliable = int(S[t:].sum())
    found = int(S[t:, 1:].sum())
    return reliable, found, ("%.6f" % (found / reliable) if reliable else "NA")


def report(k, S_draft, asm_draft, S_pol, asm_pol, reliable_min=None):
    """the file: reliable_min None = the valley of the read histogram (which both spectra share)"""
    h = histogram(S_draft)
    assert (h == histogram(S_pol)).all()
    t = valley(h) if reliable_min is None else int(reliable_min)
    lines = [f"##hypo-qv-spectra\tk={k}\treads_distinct={int(h.sum())}\treliable_min={t}\t{'valley' if reliable_min is None else 'given'}", TEXT_HEADER]
    for name, S, asm in (("draft", S_draft, asm_draft), ("polished", S_pol, asm_pol)):
        reliable, found, text = completeness(S, t)
        lines.append(f"{name}\t{reliable}\t{found}\t{text}\t{asm}")
    lines.append(COLUMNS)
    for c in range(1, CAP + 1):
        lines.append("\t".join(str(int(x)) for x in [c] + list(S_draft[c]) + list(S_pol[c])))
    return "\n".join(lines) + "\n"


def report_for(reads, k, draft_seqs, polished_seqs, reliable_min=None):
    """the file from the inputs: reads as read_counts takes them, the two lists of contig texts (the draft as PackedSeq gives it)"""
    keys, counts = read_counts(reads, k)
    d_cn, d_asm = copy_numbers([qc.draft_text(s) for s in draft_seqs], k, keys)
    p_cn, p_asm = copy_numbers(polished_seqs, k, keys)
    return report(k, spectrum(counts, d_cn), d_asm, spectrum(counts, p_cn), p_asm, reliable_min)


def info_line(path, text):
    """the line `hypo` prints on stdout for the file `text` written to `path`"""
    r = parse_report(text)
    return (f"[Hypo::Hypo] Info: spectra {path} (k = {r['k']}, reliable >= {r['reliable_min']}): "
            f"completeness draft {r['texts']['draft'][2]}, polished {r['texts']['polished'][2]}")


def parse_report(text):
    """{k, reads_distinct, reliable_min, how, texts: {name: (reliable, found, completeness as printed, asm_only_windows)},
    draft: i64[256, 5], polished: i64[256, 5]}"""
    lines = text.split("\n")
    assert lines[-1] == "" and len(lines) == 5 + CAP + 1, len(lines)
    head = lines[0].split("\t")
    assert head[0] == "##hypo-qv-spectra" and len(head) == 5 and head[4] in ("valley", "given"), lines[0]
    kv = dict(f.split("=") for f in head[1:4])
    out = {"k": int(kv["k"]), "reads_distinct": int(kv["reads_distinct"]), "reliable_min": int(kv["reliable_min"]), "how": head[4], "texts": {}}
    assert lines[1] == TEXT_HEADER and lines[4] == COLUMNS
    for name, l in zip(("draft", "polished"), lines[2:4]):
        f = l.split("\t")
        assert len(f) == 5 and f[0] == name, l
        out["texts"][name] = (int(f[1]), int(f[2]), f[3], int(f[4]))
    S = np.zeros((2, CAP + 1, COLS), np.int64)
    for c, l in enumerate(lines[5:-1], start=1):
        f = [int(x) for x in l.split("\t")]
        assert len(f) == 1 + 2 * COLS and f[0] == c, l
        S[0, c], S[1, c] = f[1:1 + COLS], f[1 + COLS:]
    out["draft"], out["polished"] = S[0], S[1]
    return out
