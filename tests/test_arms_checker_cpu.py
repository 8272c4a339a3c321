"""CPU: the plain restatement of arm selection (tests/arms_checker.py) against the C++ host loops (Alignment::find_short_arms /
find_long_arms, Contig::fill_short_windows / fill_long_windows through hypo_host_short_arms / hypo_host_long_arms) on every case of
tests/arms_cases.py — the inputs tests/test_gpu_arms_direct.py hands the kernels.  The host loops are pinned to the reference by the
end-to-end goldens and the --host-arms runs; this makes the Python text the same function on exactly these inputs.  Every case's
condition (what makes it worth running) and the consistency of its tables are checked here too."""
import os

import pytest

import arms_cases as cases
import arms_checker as ac
from hypo_amd import capi


@pytest.fixture(scope="module")
def host():
    from hypo_amd.host import HostMirror
    if not os.path.exists(capi.LIB_PATH):
        capi.build_library()
    return HostMirror()


def assert_same(c, x, valid, counts, texts):
    """field for field; the first difference is reported with its region, the type of the window and, for an arm, the alignment it is from"""
    R = c.regions
    where = lambda w: f"region {w} ({ac.TYPE_NAMES[int(R.type[w])]}, [{int(R.start[w])}, {int(R.start[w + 1])}))"
    assert len(valid) == R.n_regions
    at = 0
    by_region = {v["region"]: i for i, v in enumerate(x.windows)}
    for w in range(R.n_regions):
        if bool(valid[w]) != bool(x.region_valid[w]):
            raise AssertionError(f"{where(w)}: the host {'keeps' if valid[w] else 'drops'} the window, the checker does not; the checker's counts {x.trace['windows'].get(w)}")
        if not valid[w]:
            continue
        v = x.windows[by_region[w]]
        want = (v["n_internal"], v["n_prefix"], v["n_suffix"], v["n_empty"])
        if tuple(int(n) for n in counts[w]) != want:
            raise AssertionError(f"{where(w)}: the host counts internal / prefix / suffix / empty {counts[w].tolist()}, the checker {list(want)}")
        host_arms, mine = texts[at].split("|"), ac.window_text(R.contig4, int(R.start[w]), int(R.start[w + 1]), x.arms[by_region[w]]).split("|")
        at += 1
        assert host_arms[0] == mine[0], f"{where(w)}: the draft differs"
        origin = x.trace["windows"][w]["kept_from"]
        for j, (h, m) in enumerate(zip(host_arms[1:], mine[1:])):
            if h != m:
                raise AssertionError(f"{where(w)}: arm {j} ({m[0]}, from alignment {origin[j][1]} at [{int(c.reads.rb[origin[j][1]])}, {int(c.reads.re[origin[j][1]])})) "
                                     f"is {h[2:]} on the host, {m[2:]} in the checker")
        assert len(host_arms) == len(mine)
    assert at == len(texts)


@pytest.mark.parametrize("name", cases.CASES)
def test_the_checker_equals_the_host_loops(host, name):
    c = cases.case(name)                                       # (check_tables ran when the case was built)
    x = cases.expected(name)
    valid, counts, texts = (host.long_arms if c.long_mode else host.short_arms)(c.regions, c.reads)
    assert_same(c, x, valid, counts, texts)
    assert len(x.arms2) == sum((n + 3) // 4 for n in x.arm_len) and x.summary["n_arms"] == sum(len(a) for a in x.arms)


@pytest.mark.parametrize("name", cases.CASES)
def test_the_case_reaches_what_it_is_there_for(name):
    cases.check_tables(cases.case(name))
    reached = cases.condition(name)
    print(name, reached)


def test_check_tables_refuses_a_window_without_its_anchor():
    """a WS in front of a window, an SR of rank 0 that a window anchors on, an anchor that is not the SR's k-mer, a CIGAR that disagrees"""
    import numpy as np
    c = cases.case("corners")
    R = c.regions
    w = int(np.nonzero(R.type[:R.n_regions] == ac.OTHER)[0][0])
    for spoil in ("type", "rank", "anchor", "cigar"):
        rtype, info, anchors, cigar = R.type.copy(), R.info.copy(), R.anchor_kmers.copy(), c.reads.cigar.copy()
        if spoil == "type":
            rtype[w] = ac.WS
        sr = int(np.nonzero((R.type[:R.n_regions] == ac.SR) & (R.info[:R.n_regions] > 0))[0][1])
        if spoil == "rank":
            info[sr] = 0
        if spoil == "anchor":
            anchors[2 * int(info[sr])] ^= 1
        if spoil == "cigar":
            cigar[int(np.nonzero((cigar & 15) == 0)[0][0])] += 16
        bad = c._replace(regions=R._replace(type=rtype, info=info, anchor_kmers=anchors), reads=c.reads._replace(cigar=cigar))
        with pytest.raises(AssertionError):
            cases.check_tables(bad)
