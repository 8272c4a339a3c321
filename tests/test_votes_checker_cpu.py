"""CPU: the plain restatement of the support votes (tests/votes_checker.py) against the C++ host loops (Alignment::
update_solidkmers_support / update_minimisers_support through hypo_host_kmer_votes / hypo_host_minimizer_votes) on every case of
tests/votes_cases.py — the inputs tests/test_gpu_votes_direct.py hands the kernels.  The host loops are pinned to the reference by
the end-to-end goldens; this makes the Python text the same function on exactly these inputs.  Every case's condition (what makes it
worth running) is checked here too."""
import os

import numpy as np
import pytest

import votes_cases as cases
from hypo_amd import capi


@pytest.fixture(scope="module")
def host():
    from hypo_amd.host import HostMirror
    if not os.path.exists(capi.LIB_PATH):
        capi.build_library()
    return HostMirror()


def assert_same(what, got, want, pos=None):
    """element for element; a difference is reported with its first index, the position of that entry and both values"""
    assert got.shape == want.shape, f"{what}: {got.shape} entries, expected {want.shape}"
    bad = np.nonzero(got != want)[0]
    if bad.size:
        i = int(bad[0])
        at = "" if pos is None else f" (position {int(pos[i])})"
        raise AssertionError(f"{what}: {bad.size} of {got.size} entries differ, the first at index {i}{at}: {int(got[i])}, expected {int(want[i])}")


@pytest.mark.parametrize("name", sorted(cases.KMER_CASES))
def test_kmer_votes_of_the_checker_equal_the_host_loop(host, name):
    c = cases.kmer_case(name)
    cov, sup, _ = cases.kmer_expected(name)
    r = c.reads
    hcov, hsup = host.kmer_votes(c.k, c.total_len, c.spos, c.kids, r.rb, r.re, r.qae, r.seq_off, r.reads2)
    assert_same("coverage", cov, hcov, c.spos)
    assert_same("support", sup, hsup, c.spos)
    cases.kmer_condition(name)


@pytest.mark.parametrize("name", sorted(cases.MIN_CASES))
def test_minimizer_votes_of_the_checker_equal_the_host_loop(host, name):
    c = cases.min_case(name)
    cov, sup = cases.min_expected(name)
    r = c.reads
    hcov, hsup = host.minimizer_votes(c.tables, r.rb, r.re, r.qae, r.seq_off, r.reads2, c.read_contig)
    pos, _ = cases.entry_positions(c.tables)
    assert_same("coverage", cov, hcov, pos)
    assert_same("support", sup, hsup, pos)
    cases.min_condition(name)


def test_the_original_entries_of_the_long_reads_do_not_see_the_appended_short_reads():
    """tiles64_plus_short is tiles64 with short reads behind the last long read: the counters in front of them are the same"""
    n = cases.n_original_entries(cases.kmer_case("tiles64"))
    a, b = cases.kmer_expected("tiles64"), cases.kmer_expected("tiles64_plus_short")
    assert n > 9000 and (a[0][:n] == b[0][:n]).all() and (a[1][:n] == b[1][:n]).all()
    assert not a[0][n:].any() and b[0][n:].any()


def test_the_checker_at_32_bits_is_another_function_only_beyond_16_bit_spans():
    """wide = True changes nothing for reads that span less than 65 536 bases"""
    from votes_checker import minimizer_votes
    c = cases.min_case("geometry")
    r = c.reads
    cov, sup = minimizer_votes(c.tables, r.rb, r.re, r.qae, r.seq_off, r.reads2, c.read_contig, wide=True)
    want = cases.min_expected("geometry")
    assert (cov == want[0]).all() and (sup == want[1]).all()
