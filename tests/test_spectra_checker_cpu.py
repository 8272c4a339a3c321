"""CPU: the checker of `hypo --qv-spectra` (tests/spectra_checker.py) against a brute-force dictionary of Python strings on tiny
inputs, and the hand-made cases of the contract: short records, N and lower case, palindromes, saturation at 255, the copy-number
columns, the valley rule, NA, and the file through its own parser."""
import collections

import numpy as np
import pytest

import spectra_checker as spc

COMP = str.maketrans("ACGT", "TGCA")


def brute(seqs, k):
    """{canonical k-mer as a string: windows}, by the contract's words alone"""
    out = collections.Counter()
    for s in seqs:
        s = s.decode().upper()
        for i in range(len(s) - k + 1):
            w = s[i:i + k]
            if set(w) <= set("ACGT"):
                out[min(w, w.translate(COMP)[::-1])] += 1
    return out


def code(w):
    return sum("ACGT".index(c) << (2 * (len(w) - 1 - i)) for i, c in enumerate(w))


def as_dict(keys, values, k):
    return {int(x): int(v) for x, v in zip(keys, values)}


def rnd(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(list(alphabet), n).astype(np.uint8))


@pytest.mark.parametrize("k", [12, 13, 21, 22, 31])
def test_against_brute_force(k):
    rng = np.random.default_rng(k)
    base = rnd(rng, 300)
    reads = [base[i:i + 80] for i in range(0, 220, 7)] + [rnd(rng, 60, b"ACGTN"), rnd(rng, 50, b"ACGTacgtn"), base[:100].lower(), b"", rnd(rng, k - 1), rnd(rng, k)]
    reads += [r.decode().translate(COMP)[::-1].encode() for r in reads[:10]]
    texts = [base, base[50:120] * 3, rnd(rng, 90), base[200:260] + b"N" + base[200:260]]
    keys, counts = spc.read_counts(reads, k)
    want = brute(reads, k)
    assert as_dict(keys, counts, k) == {code(w): min(c, 255) for w, c in want.items()}
    cn, asm_only = spc.copy_numbers(texts, k, keys)
    tw = brute(texts, k)
    assert as_dict(keys, cn, k) == {code(w): min(tw.get(w, 0), 255) for w in want}
    assert asm_only == sum(c for w, c in tw.items() if w not in want)
    S = spc.spectrum(counts, cn)
    for c in range(256):
        for j in range(5):
            assert S[c, j] == sum(1 for w, n in want.items() if min(n, 255) == c and min(tw.get(w, 0), 4) == j)
    assert S.sum() == len(want) and not S[0].any()


def test_short_records_n_and_case():
    k = 12
    keys, counts = spc.read_counts([b"ACGTACGTACG", b"", b"ACGTACGTAC"], k)          # 11, 0 and 10 bases: no window
    assert keys.size == 0 and counts.size == 0
    # the two records do not join into one run, an N ends one, and case does not matter
    a, b = b"ACGGTCATTGCA", b"TTGACCGTAGCA"
    keys, counts = spc.read_counts([a, b], k)
    assert sorted(as_dict(keys, counts, k).items()) == sorted({code(min(w, w.translate(COMP)[::-1])): 1 for w in (a.decode(), b.decode())}.items())
    one = spc.read_counts([a + b], k)
    assert one[0].size == 13
    assert spc.read_counts([a[:6] + b"N" + a[6:]], k)[0].size == 0
    lower = spc.read_counts([a.lower() + b"n" + b.lower(), a], k)
    assert as_dict(*lower, k) == {code(min(w, w.translate(COMP)[::-1])): n for w, n in ((a.decode(), 2), (b.decode(), 1))}


@pytest.mark.parametrize("k", [12, 22])
def test_a_palindrome_counts_once(k):
    half = "ACGTTGCAAGCTTAGG"[:k // 2]
    pal = half + half.translate(COMP)[::-1]
    assert pal == pal.translate(COMP)[::-1] and len(pal) == k
    keys, counts = spc.read_counts([pal.encode()], k)
    assert as_dict(keys, counts, k) == {code(pal): 1}
    keys, counts = spc.read_counts([pal.encode(), b"GG" + pal.lower().encode() + b"N"], k)
    assert counts[list(keys).index(code(pal))] == 2
    cn, asm_only = spc.copy_numbers([pal], k, keys)
    assert cn[list(keys).index(code(pal))] == 1 and asm_only == 0


def test_counts_stop_at_255():
    k = 20
    keys, counts = spc.read_counts([b"A" * 300], k)                                   # 281 windows
    assert as_dict(keys, counts, k) == {0: 255}
    cn, asm_only = spc.copy_numbers([b"T" * 300, b"A" * 30], k, keys)                 # 281 + 11 windows of the same canonical k-mer
    assert cn.tolist() == [255] and asm_only == 0
    assert spc.spectrum(counts, cn)[255].tolist() == [0, 0, 0, 0, 1]


def test_copy_number_columns():
    """a k-mer 3 times in the text, others 4 and 6 times: columns 3, 4 and 4"""
    k = 12
    rng = np.random.default_rng(5)
    x, y, z, w = (rnd(rng, k) for _ in range(4))
    reads = [x, x, y, z, z, z, w]
    text = b"N".join([x] * 3 + [y] * 4 + [z] * 6 + [rnd(rng, k)])
    keys, counts = spc.read_counts(reads, k)
    cn, asm_only = spc.copy_numbers([text], k, keys)
    assert asm_only == 1
    S = spc.spectrum(counts, cn)
    want = np.zeros((256, 5), np.int64)
    want[2, 3] = 1          # x: twice in the reads, 3 times in the text
    want[1, 4] += 1         # y: once, 4 times
    want[3, 4] = 1          # z: 3 times, 6 times
    want[1, 0] += 1         # w: once, not in the text
    assert (S == want).all()


def test_valley_rule():
    h = np.zeros(256, np.int64)
    h[1:8] = [900, 300, 80, 20, 25, 60, 200]            # falls until 4, rises from 4 to 5
    assert spc.valley(h) == 4
    h2 = np.zeros(256, np.int64)
    h2[1:6] = [50, 10, 10, 40, 90]                      # a tie counts: h[2] <= h[3]
    assert spc.valley(h2) == 2
    mono = np.arange(1000, 1000 - 256, -1, dtype=np.int64)      # strictly falling all the way: no valley
    assert spc.valley(mono) == 2
    late = mono.copy()
    late[255] = late[254]                               # c = 254 is the last place looked at
    assert spc.valley(late) == 254
    first = mono.copy()
    first[1] = 0                                        # h[1] <= h[2] is not looked at
    assert spc.valley(first) == 2


def test_completeness_and_na():
    S = np.zeros((256, 5), np.int64)
    S[1] = [100, 3, 0, 0, 0]
    S[5] = [2, 10, 1, 0, 0]
    S[255] = [0, 0, 0, 0, 1]
    assert spc.completeness(S, 2) == (14, 12, "%.6f" % (12 / 14))
    assert spc.completeness(S, 1) == (117, 15, "%.6f" % (15 / 117))
    assert spc.completeness(S, 6) == (1, 1, "1.000000")
    assert spc.completeness(np.zeros((256, 5), np.int64), 2) == (0, 0, "NA")
    S[255] = 0
    assert spc.completeness(S, 6) == (0, 0, "NA")


def test_file_round_trips():
    rng = np.random.default_rng(9)
    k = 15
    genome = rnd(rng, 2000)
    reads = [genome[i:i + 100] for i in rng.integers(0, 1900, 400)]
    draft = genome[:700] + b"n" + genome[700:1500] + genome[1200:1500]
    polished = genome[:1990]
    text = spc.report_for(reads, k, [draft.decode()], [polished.decode()])
    r = spc.parse_report(text)
    keys, counts = spc.read_counts(reads, k)
    assert (r["k"], r["reads_distinct"], r["how"]) == (k, keys.size, "valley")
    assert r["reliable_min"] == spc.valley(spc.histogram(r["draft"])) >= 2
    assert (spc.histogram(r["draft"]) == spc.histogram(r["polished"])).all() and spc.histogram(r["draft"]).sum() == keys.size
    assert r["polished"][:, 2:].sum() == 0 and r["draft"][:, 2].sum() > 200
    for name in ("draft", "polished"):
        reliable, found, printed, asm_only = r["texts"][name]
        assert (reliable, found, printed) == spc.completeness(r[name], r["reliable_min"])
    in_reads = brute(reads, k)
    for name, t in (("draft", draft.replace(b"n", b"N")), ("polished", polished)):
        assert r["texts"][name][3] == sum(c for w, c in brute([t], k).items() if w not in in_reads)
    assert text == spc.report(k, r["draft"], r["texts"]["draft"][3], r["polished"], r["texts"]["polished"][3])
    given = spc.report_for(reads, k, [draft.decode()], [polished.decode()], reliable_min=7)
    g = spc.parse_report(given)
    assert (g["reliable_min"], g["how"]) == (7, "given") and g["texts"]["draft"][:3] == spc.completeness(r["draft"], 7)
    assert text.count("\n") == 5 + 255 and text.split("\n")[5].startswith("1\t") and text.split("\n")[259].startswith("255\t")
    assert "completeness draft " + r["texts"]["draft"][2] in spc.info_line("x.tsv", text)
    empty = spc.parse_report(spc.report_for([b"ACGT"], k, ["ACGT"], ["ACGT"]))
    assert empty["texts"]["draft"] == (0, 0, "NA", 0) and empty["reliable_min"] == 2
