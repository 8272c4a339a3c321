"""CPU: tests/cn_checker.py pinned on cases computed by hand (k = 3, so that every code can be written down): the windows and their
canonical codes, the bins, the six columns with an odd and an even number of present windows, an all-missing bin, saturated c and m,
m = 0, `over` and `under` exactly at their thresholds, valley and peak, the file and the Info line."""
import pytest

import cn_checker as cn

# ACGTTGCA, k = 3: ACG / CGT -> 6 (ACG), GTT -> 1 (AAC), TTG -> 16 (CAA), TGC / GCA -> 36 (GCA)
SEQ = "ACGTTGCA"
CODES = [6, 6, 1, 16, 36, 36]


def test_windows_and_codes():
    assert cn.windows(SEQ, 3) == list(enumerate(CODES))
    assert cn.windows("acgttgca", 3) == list(enumerate(CODES))                      # lower case
    assert cn.windows("ACGNACG", 3) == [(0, 6), (4, 6)]                             # no window over the N
    assert cn.windows("AC", 3) == [] and cn.windows("", 3) == []
    assert cn.tally([SEQ, "ACG"], 3) == {6: 3, 1: 1, 16: 1, 36: 2}
    assert cn.tally(["A" * 400], 3) == {0: 255}                                     # stops at 255


def test_bins():
    assert [cn.n_bins(n, 4) for n in (0, 1, 3, 4, 5, 8, 9)] == [0, 1, 1, 1, 2, 2, 3]
    # a sequence shorter than k still has its bin, all zeros; an empty one has none
    d = cn.depth(["AC", "", SEQ], 3, 4, {6: 1}, {6: 1}, 1)
    assert d["windows"] == [0, 4, 2] and d["missing"] == [0, 2, 2] and d["med_count"] == [0, 1, 0]


def test_columns_even_present():
    d = cn.depth([SEQ], 3, 4, {6: 10, 1: 4, 16: 7, 36: 20}, {6: 2, 1: 1, 16: 1, 36: 2}, 10)
    # bin 0: c = 10, 10, 4, 7 against m = 2, 2, 1, 1 at 10 reads a copy: all four at most 0.75 of what their copies ask
    assert d == {"windows": [4, 2], "missing": [0, 0], "rated": [4, 2], "over": [0, 0], "under": [4, 0], "med_count": [7, 20]}


def test_thresholds_exactly():
    # unit 4, m = 1: over from 2 c >= 12 (c = 6 is, c = 5 is not), under up to 4 c <= 12 (c = 3 is, c = 4 is not)
    d = cn.depth([SEQ], 3, 4, {6: 6, 1: 5, 16: 3, 36: 4}, {6: 1, 1: 1, 16: 1, 36: 1}, 4)
    assert d == {"windows": [4, 2], "missing": [0, 0], "rated": [4, 2], "over": [2, 0], "under": [1, 0], "med_count": [5, 4]}
    # unit 2, m = 3: over from 2 c >= 18, under up to 4 c <= 18
    d = cn.depth(["ACG"], 3, 4, {6: 9}, {6: 3}, 2)
    assert (d["over"], d["under"]) == ([1], [0])
    d = cn.depth(["ACG"], 3, 4, {6: 8}, {6: 3}, 2)
    assert (d["over"], d["under"]) == ([0], [0])
    d = cn.depth(["ACG"], 3, 4, {6: 4}, {6: 3}, 2)
    assert (d["over"], d["under"]) == ([0], [1])
    d = cn.depth(["ACG"], 3, 4, {6: 5}, {6: 3}, 2)
    assert (d["over"], d["under"]) == ([0], [0])


def test_saturated_unmarked_missing_and_odd_present():
    reads, text = {6: 255, 1: 1, 16: 9}, {6: 3, 1: 255}
    # t = 2: code 1 (seen once) is missing, 36 is not among the reads; present c = 255, 255, 9 (odd: the median is the 2nd of 3);
    # c = 255 cannot be rated, and code 16 has m = 0
    d = cn.depth([SEQ], 3, 4, reads, text, 5, t=2)
    assert d == {"windows": [4, 2], "missing": [1, 2], "rated": [0, 0], "over": [0, 0], "under": [0, 0], "med_count": [255, 0]}
    # t = 1: code 1 is present, but its m = 255 cannot be rated; four present: the lower median is the 2nd of 1, 9, 255, 255
    d = cn.depth([SEQ], 3, 4, reads, text, 5, t=1)
    assert d == {"windows": [4, 2], "missing": [0, 2], "rated": [0, 0], "over": [0, 0], "under": [0, 0], "med_count": [9, 0]}
    # m = 254 and c = 254 are the last that can be rated
    d = cn.depth(["ACG"], 3, 4, {6: 254}, {6: 254}, 1)
    assert (d["rated"], d["over"], d["under"]) == ([1], [0], [0])
    d = cn.depth(["ACG"], 3, 4, {6: 254}, {6: 255}, 1)
    assert d["rated"] == [0]


def test_valley_and_peak():
    h = [0] * 256
    h[1:8] = [100, 50, 20, 30, 60, 60, 10]
    assert cn.valley(h) == 3 and cn.peak(h) == 5                                    # the smaller of two equal tops
    assert cn.valley([0] * 256) == 2 and cn.peak([0] * 256) == 0
    h = [0] * 256
    h[255] = 1000                                                                   # 255 says "at least": no peak
    assert cn.peak(h) == 0
    h[1], h[2] = 500, 3                                                             # the error k-mers below the valley do not count
    assert cn.valley(h) == 3 and cn.peak(h) == 0
    h[254] = 1
    assert cn.peak(h) == 254
    assert cn.histogram({1: 3, 2: 3, 9: 255})[3] == 2


FILE = ("##hypo-qv-cn\tk=3\tbin=4\tunit=10\tgiven\tmin_count=1\n"
        "#contig\tstart\tend\twindows\tmissing\trated\tover\tunder\tmedian_count\tcall\n"
        "short\t0\t2\t0\t0\t0\t0\t0\t0\t.\n"
        "ctg\t0\t4\t4\t0\t4\t0\t4\t7\tduplicated\n"
        "ctg\t4\t8\t2\t0\t2\t0\t0\t20\t.\n")


def test_file_and_info_line():
    reads, text = {6: 10, 1: 4, 16: 7, 36: 20}, {6: 2, 1: 1, 16: 1, 36: 2}
    got = cn.report(["short", "none", "ctg"], ["AC", "", SEQ], 3, 4, reads, text, unit=10)
    assert got == FILE
    r = cn.parse_report(got)
    assert (r["k"], r["bin"], r["unit"], r["how"], r["min_count"]) == (3, 4, 10, "given", 1)
    assert r["rows"][1] == ("ctg", 0, 4, 4, 0, 4, 0, 4, 7, "duplicated")
    assert cn.info_line("cn.tsv", got) == ("[Hypo::Hypo] Info: copy number cn.tsv (k = 3, bin = 4, unit = 10 given): 3 bins, "
                                            "0 collapsed (0 bases), 1 duplicated (4 bases)")
    assert cn.call(4, 3, 0) == "collapsed" and cn.call(4, 2, 2) == "." and cn.call(0, 0, 0) == "." and cn.call(5, 0, 3) == "duplicated"
    # the default unit is the peak of the read histogram, and a histogram without one is an error
    reads = {c: 20 for c in range(40)}
    reads.update({100 + c: 1 for c in range(90)})
    assert cn.report(["ctg"], [SEQ], 3, 4, reads, {}, unit=None).startswith("##hypo-qv-cn\tk=3\tbin=4\tunit=20\tpeak\tmin_count=1\n")
    with pytest.raises(ValueError):
        cn.report(["ctg"], [SEQ], 3, 4, {6: 255}, {}, unit=None)
