"""Generator of "growing" LONG windows: windows whose round-1 consensus is NOT about as long as the draft (test infrastructure).

A LONG window is polished in two rounds (src/Window.cpp:156-254) and the second round aligns the arms against the first round's curated
consensus, not against the draft.  Simulator windows and the goldens have a consensus about as long as the draft, so every capacity that
is sized from "draft + arms" is exercised only where it cannot be wrong.  The families here move the consensus away from the draft:

    own_ins        draft 60-400; 2-3 internal arms, each the draft plus its OWN random 20-200-base insertion at its own place.  n_internal
                   <= 3 makes curate's threshold floor(0.4 * n_internal) 0 or 1: (next to) nothing is curated, the consensus is longer than
                   the draft and may be longer than every arm.
    shared_ins     draft 100-600; 5-9 arms, at least 60 % of them carry the same insertion of 0.2-3 x the draft length (0.5-1.5 % noise),
                   the rest are the draft with 2-4 % noise: the consensus is far longer than the draft and survives curate.
    stacked        draft 300-700.  Two windows of three: three places, three groups of 2-3 full-length arms, the 70-150-base insertion at
                   place k is carried by groups k and k + 1 (of three): 2 g carriers against g arms without it and the draft, so every
                   arm carries two of the insertions and the heaviest path all three — the consensus is longer than EVERY sequence of the
                   window, by one insertion, i.e. by more than the 66 bases beyond which class 6's sequence buffer, once sized as the longest
                   sequence + 64, was overrun.  No search over seeds is needed: about 14 of 16 such windows reach it (a zero-length arm
                   raises the threshold in the others).  The third window: 1 full-length arm and, for each of 2 stretches of the draft,
                   3 arms that cover that stretch only and carry an insertion in it.  (kNW charges such an arm one end gap per uncovered
                   node wherever its ends lie, so its last base ties between its own place and the last node of its letter, the traceback
                   prefers the diagonal there, and three such arms make a heavy edge that SKIPS the rest of the draft: the consensus of
                   these windows is shorter than the draft, in the reference as in the oracle.  They stay as a shape of their own.)
    shrink         control: 5-9 arms, at least 60 % of them lack a stretch of 20-60 % of the draft: consensus far shorter than the draft.
    prefix_suffix  windows of the families above with some arms handed over as prefix / suffix arms: a LONG window aligns every kind as
                   kNW (src/Window.cpp:166-207 changes the type of the SHORT engine and aligns with the LONG one), and n_internal, so
                   the threshold, shrinks.
    giant          shared_ins with a 500-base draft and a 1 500-3 000-base insertion in 7 of 9 arms, and with a 1 300-base draft: only
                   size class 6 holds them (classes 4 / 5 end at sequences of 1 021 bases).

A few windows carry zero-length arms and n_empty > 0.  Every window is emitted twice: as generated, and with some bases of its draft
replaced by N.

The real reference filters the arms of a LONG window as they are added (Filter::is_good, include/Filter.hpp:64-102: at least one
minimizer shared with the draft per 50 bases of the arm).  The arms here pass it by construction — the draft-derived part of a carrier arm
keeps nearly all of the draft's minimizers, and where the insertion is longer than about 3 x the draft (giant) it carries exact copies of
short draft stretches between its random blocks, as a tandem duplication would — and the tests assert the share the reference reports as
filtered (at most 5 % per family) rather than assume it.

    windows(family, seed, n, small=False)  ->  list of 2 * n hypo_amd.batch.TextWindow (each window followed by its N twin), is_long = True
"""
import numpy as np

from hypo_amd.batch import TextWindow

FAMILIES = ("own_ins", "shared_ins", "stacked", "shrink", "prefix_suffix", "giant")
_A = "ACGT"


def _rnd(rng, n):
    return "".join(_A[i] for i in rng.integers(0, 4, size=int(n)))


def _noisy(rng, s, err):
    """s with `err` errors per base: a third each substitutions, deletions, insertions."""
    out = []
    for ch in s:
        r = rng.random()
        if r < err / 3:
            continue
        out.append(_A[rng.integers(0, 4)] if r < 2 * err / 3 else ch)
        if rng.random() < err / 3:
            out.append(_A[rng.integers(0, 4)])
    return "".join(out) or "A"


def _with_n(rng, w):
    """The window with 1-3 bases of its draft replaced by N (short drafts: one)."""
    d = list(w.draft)
    for p in rng.choice(len(d), size=min(len(d), int(rng.integers(1, 4)) if len(d) >= 40 else 1), replace=False):
        d[int(p)] = "N"
    return TextWindow("".join(d), list(w.internal), list(w.prefix), list(w.suffix), w.n_empty, True)


def _insertion(rng, draft, n):
    """n bases to insert.  Up to 3 x the draft: random.  Beyond: random blocks of 60 bases with a 24-base copy of a draft stretch behind
    each, so that the arm keeps one shared minimizer per 50 bases (module docstring)."""
    if n <= 3 * len(draft) or len(draft) < 48:
        return _rnd(rng, n)
    out, have = [], 0
    while have < n:
        p = int(rng.integers(0, len(draft) - 24))
        blk = _rnd(rng, 60) + draft[p:p + 24]
        out.append(blk)
        have += len(blk)
    return "".join(out)[:n]


def _own_ins(rng, small=False):
    d = _rnd(rng, rng.integers(60, 141 if small else 401))
    arms = []
    for _ in range(int(rng.integers(2, 4))):
        p = int(rng.integers(0, len(d) + 1))
        arms.append(d[:p] + _rnd(rng, rng.integers(20, 81 if small else 201)) + d[p:])
    return TextWindow(d, arms, [], [], 0, True)


def _shared_ins(rng, small=False, dlen=None, ins_len=None, n_arms=None, n_carriers=None):
    d = _rnd(rng, dlen if dlen is not None else rng.integers(100, 161 if small else 601))
    n = int(n_arms if n_arms is not None else rng.integers(5, 7 if small else 10))
    c = int(n_carriers if n_carriers is not None else rng.integers(-(-6 * n // 10), n + 1))
    il = int(ins_len if ins_len is not None else rng.uniform(0.2, 1.2 if small else 3.0) * len(d))
    p = int(rng.integers(len(d) // 5, 4 * len(d) // 5 + 1))
    grown = d[:p] + _insertion(rng, d, il) + d[p:]
    carrier = np.zeros(n, dtype=bool)
    carrier[rng.choice(n, size=c, replace=False)] = True
    arms = [_noisy(rng, grown, rng.uniform(0.005, 0.015)) if carrier[i] else _noisy(rng, d, rng.uniform(0.02, 0.04)) for i in range(n)]
    return TextWindow(d, arms, [], [], 0, True)


def _stacked(rng, small=False, i=0):
    d = _rnd(rng, rng.integers(240, 281) if small else rng.integers(300, 701))
    if i % 3 == 2:
        # arms that cover a stretch of the draft only (kNW: the rest of the graph is one end gap on either side) and carry an insertion in it
        half = len(d) // 2
        arms = [_noisy(rng, d, 0.01)]
        for k in range(2):
            mid = k * half + half // 2 + int(rng.integers(-15, 16))
            ins = _rnd(rng, rng.integers(45, 91))
            for _ in range(3):
                fl, fr = int(rng.integers(85, 101)), int(rng.integers(85, 101))
                arms.append(d[mid - fl:mid] + ins + d[mid:mid + fr])
    else:
        # three places, three groups of g arms: the insertion at place k is in the arms of groups k and k + 1 (of three) — 2 g carriers
        # against the g arms without it and the draft — so every arm carries two of the three insertions and the consensus all three
        g = 2 if small else int(rng.integers(2, 4))
        place = sorted(int(x) for x in rng.choice(np.arange(20, len(d) - 20), size=3, replace=False))
        ins = [_rnd(rng, rng.integers(70, 81 if small else 151)) for _ in range(3)]
        arms = []
        for grp in range(3):
            for _ in range(g):
                t, at = d, 0
                out = []
                for k in range(3):
                    out.append(t[at:place[k]])
                    if grp in (k, (k + 1) % 3):
                        out.append(ins[k])
                    at = place[k]
                out.append(t[at:])
                arms.append(_noisy(rng, "".join(out), 0.005))
    order = rng.permutation(len(arms))
    return TextWindow(d, [arms[j] for j in order], [], [], 0, True)


def _shrink(rng, small=False):
    d = _rnd(rng, rng.integers(130, 221) if small else rng.integers(100, 601))
    n = int(rng.integers(5, 7 if small else 10))
    c = int(rng.integers(-(-6 * n // 10), n + 1))
    cut = int(rng.uniform(0.2, 0.6) * len(d))
    p = int(rng.integers(0, len(d) - cut + 1))
    short = d[:p] + d[p + cut:]
    lacking = np.zeros(n, dtype=bool)
    lacking[rng.choice(n, size=c, replace=False)] = True
    arms = [_noisy(rng, short if lacking[i] else d, rng.uniform(0.01, 0.03)) for i in range(n)]
    return TextWindow(d, arms, [], [], 0, True)


def _prefix_suffix(rng, small=False):
    w = (_own_ins, _shared_ins, _stacked, _shrink)[int(rng.integers(0, 4))](rng, small)
    arms = list(w.internal)
    kind = rng.integers(0, 3, size=len(arms))
    kind[int(rng.integers(0, len(arms)))] = 1 + int(rng.integers(0, 2))             # at least one arm changes its kind
    pick = lambda k: [a for a, x in zip(arms, kind) if x == k]
    return TextWindow(w.draft, pick(0), pick(1), pick(2), 0, True)


def _giant(rng, i):
    if i % 2 == 0:
        return _shared_ins(rng, dlen=500, ins_len=int(rng.integers(1500, 3001)), n_arms=9, n_carriers=7)
    return _shared_ins(rng, dlen=1300, ins_len=int(rng.integers(300, 1301)), n_arms=int(rng.integers(5, 8)))


def windows(family, seed, n, small=False):
    """2 * n windows of a family, deterministic in (family, seed, n, small): window, its twin with N in the draft, window, twin, ...
    small: the same shapes drawn from the low end of every range (the lockstep emulator of class 6 takes seconds per full-size window)."""
    rng = np.random.default_rng([FAMILIES.index(family), int(seed), int(small)])
    out = []
    for i in range(n):
        if family == "giant":
            w = _giant(rng, i)
        else:
            w = _stacked(rng, small, i) if family == "stacked" else {"own_ins": _own_ins, "shared_ins": _shared_ins, "shrink": _shrink, "prefix_suffix": _prefix_suffix}[family](rng, small)
            if i % 8 == 5:                                   # a zero-length arm among the others (it is counted, never aligned) ...
                w.internal.insert(int(rng.integers(0, len(w.internal) + 1)), "")
            if i % 8 == 6 and w.suffix:
                w.suffix.append("")
            if i % 8 == 7:                                   # ... and arms that were empty before they were packed
                w.n_empty = int(rng.integers(1, 3))
        out.append(w)
        out.append(_with_n(rng, w))
    return out
