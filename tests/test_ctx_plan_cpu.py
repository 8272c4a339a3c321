"""CPU: how a contig batch is dealt out to the device contexts (hypo_amd/csrc/host/CtxPlan.hpp, through hypo_host_plan_contexts).
The expected values were worked out by hand from the code as it stood inside Hypo::polish before it became a function of its own:
contiguous ranges of about equal numbers of alignments (+ 1 per contig) when the batch has at least as many contigs as contexts,
coordinate ranges of the contigs ("pieces") when it has fewer."""
import os

import pytest

from hypo_amd import capi


@pytest.fixture(scope="module")
def host():
    from hypo_amd.host import HostMirror
    if not os.path.exists(capi.LIB_PATH):
        capi.build_library()
    return HostMirror()


def test_one_context_takes_the_batch(host):
    assert host.plan_contexts(3, 8, 1, [5, 0, 7, 1, 2], [100] * 5, False, False) == [(3, 8, False, 0, 0)]


def test_host_arms_leave_the_batch_with_context_0(host):
    # several contexts, but split_batch is false (--host-arms): the other contexts get empty ranges
    assert host.plan_contexts(0, 4, 2, [4, 4, 4, 4], [100] * 4, False, True) == [(0, 4, False, 0, 0), (0, 0, False, 0, 0)]


def test_equal_shares_cut_in_the_middle(host):
    # shares 5 each, total 20: the first cut is due behind contig 1 (10 * 2 >= 20 * 1); contig ids are the draft's, not the batch's
    assert host.plan_contexts(3, 7, 2, [4, 4, 4, 4], [100] * 4, True, False) == [(3, 5, False, 0, 0), (5, 7, False, 0, 0)]


def test_tail_rule_gives_every_context_a_contig(host):
    # shares 11, 1, 1, 1, 91 of 105: half is reached only with the LAST contig, where no contig would be left for context 1; the
    # contigs behind the loop are handed out from the end
    work = host.plan_contexts(0, 5, 2, [10, 0, 0, 0, 90], [100] * 5, True, True)
    assert [(w[0], w[1]) for w in work] == [(0, 4), (4, 5)]
    assert work[0][0] == 0 and work[-1][1] == 5
    assert all(a[1] == b[0] for a, b in zip(work, work[1:])), "ranges are not contiguous"
    assert all(w[1] - w[0] >= 1 and not w[2] for w in work)


def test_fewer_contigs_than_contexts_are_cut_into_pieces(host):
    # loads 2 and 101 per context: the third context goes to contig 1 -> shares [1, 2]
    work = host.plan_contexts(0, 2, 3, [1, 100], [500, 1001], True, True)
    assert work[0][:3] == (0, 1, False)
    assert work[1] == (1, 2, True, 0, 500) and work[2] == (1, 2, True, 500, 1001)


def test_pieces_not_allowed(host):
    work = host.plan_contexts(0, 2, 3, [1, 100], [500, 1001], True, False)
    assert work[0] == (0, 2, False, 0, 0)
    assert all(w[0] == w[1] and not w[2] for w in work[1:])


def test_one_contig_on_four_contexts(host):
    work = host.plan_contexts(0, 1, 4, [1000], [10], True, True)
    assert all(w[:3] == (0, 1, True) for w in work)
    assert [w[3] for w in work] + [work[-1][4]] == [0, 2, 5, 7, 10]
    assert all(a[4] == b[3] for a, b in zip(work, work[1:]))
