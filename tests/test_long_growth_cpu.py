"""LONG windows whose consensus outgrows (or undercuts) the draft, in every size class that takes LONG windows, on the CPU.

The second round of a LONG window (src/Window.cpp:156-254) aligns against the first round's consensus, not the draft; the simulator's
windows and the goldens have a consensus about as long as the draft.  tests/long_growth.py generates the windows that do not; here they
run through the oracle, the real reference (where oracle/_ref was built), and the lockstep emulator of the device code: size class 6
(Giant::run, poa_giant.hpp), classes 4 and 5 on their own, and the re-queue chain from class 4.

Before class 6 sized its tables for the second round it answered RES_OVERFLOW for 20 of the 24 first own_ins windows, 18 of 20 shared_ins
and all giant ones (the label table, sized from "draft + arms", was full as soon as the consensus was some 20 bases longer than the draft).

Sizes: the emulator runs 64 lanes in lockstep and takes seconds per full-size window in class 6, so most windows of a family are drawn
from the low end of its ranges (long_growth.windows(..., small=True)) and a few at full size: 300 windows in all.  Last: a bounded LONG
space of tiny windows (arms of 0-4 bases), a strided sample of it, against the oracle in classes 4, 5 and 6."""
import os
import subprocess
import sys

import numpy as np
import pytest

import emu_util
import exhaustive_parity as ex
import long_growth as lg
from hypo_amd.batch import build_batch

# family: (seed, windows before the N twins, small) ...
PLAN = {
    "own_ins": [(1, 12, False), (2, 8, False), (3, 16, True), (4, 15, True)],
    "shared_ins": [(1, 3, False), (2, 8, True), (3, 4, True)],
    "stacked": [(1, 3, False), (2, 9, True), (3, 12, True)],
    "shrink": [(1, 5, False), (2, 5, False), (3, 13, True), (4, 12, True)],
    "prefix_suffix": [(1, 4, False), (2, 10, True), (3, 10, True)],
    "giant": [(1, 2, False)],              # (of these four, the 500-base draft as generated and the 1 300-base draft's N twin: GIANT_PICK)
}
GIANT_PICK = (0, 3)
SLICE = 64 << 20
OVER = (emu_util.RES_OVERFLOW, emu_util.RES_UNSUPPORTED)


def test_the_plan_holds_300_windows():
    assert sum(2 * n for name, plan in PLAN.items() for _, n, _ in plan if name != "giant") + len(GIANT_PICK) >= 300


@pytest.fixture(scope="module")
def emu():
    return emu_util.Emu()


class _Family:
    def __init__(self, family, orc):
        self.windows = [w for seed, n, small in PLAN[family] for w in lg.windows(family, seed, n, small)]
        if family == "giant":
            self.windows = [self.windows[i] for i in GIANT_PICK]
        self.batch = build_batch(self.windows)
        self.off = self.batch.slot_layout()
        self.want, self.status, self.cells, self.aligns = orc.poa_batch(self.batch, off=self.off)
        self.longest = [max([len(w.draft)] + [len(a) for a in w.internal + w.prefix + w.suffix]) for w in self.windows]
        self._giant = None

    def giant(self, emu):
        if self._giant is None:
            self._giant = emu.poa_giant(self.batch, off=self.off, slice_bytes=SLICE)
        return self._giant

    def describe(self, i):
        w = self.windows[i]
        return f"window {i}: draft {len(w.draft)}, arms {[len(a) for a in w.internal]} / {[len(a) for a in w.prefix]} / {[len(a) for a in w.suffix]}, n_empty {w.n_empty}"


_cache = {}


@pytest.fixture
def fam(request, oracle_lib):
    name = request.param
    if name not in _cache:
        _cache[name] = _Family(name, oracle_lib)
    return name, _cache[name]


families = pytest.mark.parametrize("fam", lg.FAMILIES, indirect=True)


@families
def test_the_families_are_what_they_say(fam):
    """The oracle answers every window, and the consensus is where the family puts it relative to the draft / the longest sequence."""
    name, f = fam
    assert (f.status == 0).all()
    cons = np.array([len(c) for c in f.want])
    draft = np.array([len(w.draft) for w in f.windows])
    longest = np.array(f.longest)
    if name == "own_ins":
        assert (cons > draft + 20).mean() > 0.5 and (cons > longest).any()
    elif name in ("shared_ins", "giant"):
        assert (cons > 1.15 * draft).mean() > 0.9
    elif name == "shrink":
        assert (cons < 0.85 * draft).mean() > 0.9
    elif name == "stacked":
        # the consensus is longer than EVERY sequence by more than 66 bases (a sequence buffer of "longest sequence + 64" is overrun)
        assert (cons > longest + 66).sum() >= 10
    else:
        assert all(w.prefix or w.suffix for w in f.windows)
    if name != "giant":
        assert any(w.n_empty for w in f.windows) and any("" in w.internal for w in f.windows) and all("N" in w.draft for w in f.windows[1::2])


@families
def test_oracle_vs_real_reference(fam):
    import oracle
    name, f = fam
    if not oracle.Ref.available():
        pytest.skip("oracle/_ref/libhyporef.so not built (the real reference only exists in the build container)")
    rb, _, rln, rst, _ = oracle.Ref().poa_batch_raw(f.batch, off=f.off)
    filtered = rst == oracle.REF_ST_FILTERED
    print(f"{name}: {int(filtered.sum())} of {len(f.windows)} windows FILTERED by the reference's own Window ({100 * filtered.mean():.1f} %)")
    assert filtered.mean() <= 0.05, f"{name}: the reference filtered an arm of {int(filtered.sum())} of {len(f.windows)} windows"
    for i in np.nonzero(~filtered)[0]:
        o = int(f.off[i])
        assert rst[i] == f.status[i] and rb[o:o + int(rln[i])].tobytes().decode() == f.want[i], f"{name} {f.describe(i)}"


@families
def test_class_6_vs_oracle(emu, fam):
    name, f = fam
    cons, st, res, cells, aligns = f.giant(emu)
    bad = [i for i in range(len(f.windows)) if res[i] != emu_util.RES_OK or st[i] != f.status[i] or cons[i] != f.want[i]]
    assert not bad, (f"{name}: {len(bad)} of {len(f.windows)} windows; first {f.describe(bad[0])}: class 6 result {int(res[bad[0]])} "
                     f"(1 = RES_OVERFLOW), oracle consensus {len(f.want[bad[0]])} bases")
    assert cells == f.cells and aligns == f.aligns


@families
def test_classes_4_and_5_and_the_chain_vs_oracle(emu, fam):
    name, f = fam
    n = len(f.windows)
    for cfg in (4, 5):
        cons, st, res, _, _ = emu.poa_batch(f.batch, cfg, off=f.off)
        for i in range(n):
            assert res[i] == emu_util.RES_OK or res[i] in OVER, f"{name} class {cfg} {f.describe(i)}: result {int(res[i])}"
            assert res[i] != emu_util.RES_OK or (st[i] == f.status[i] and cons[i] == f.want[i]), f"{name} class {cfg} {f.describe(i)}"
        if name == "giant":
            assert all(r in OVER for r in res), "only class 6 holds these"
    # the chain from class 4: answered in class 4 or 5, or handed on by class 5 — on the device to class 6 (poa_kernel.hip:368-376)
    cons, res, hops, _ = emu.poa_chain(f.batch, 4, off=f.off)
    g_cons, _, g_res, _, _ = f.giant(emu)
    for i in range(n):
        assert res[i] == emu_util.RES_OK or res[i] in OVER, f"{name} chain {f.describe(i)}: result {int(res[i])}"
        end = cons[i] if res[i] == emu_util.RES_OK else (g_cons[i] if g_res[i] == emu_util.RES_OK else None)
        assert end == f.want[i], f"{name} chain {f.describe(i)} (classes visited: {int(hops[i])})"


def test_class_6_answers_or_refuses_at_the_edge_of_its_slice(emu, oracle_lib):
    """Slices around what the windows need: a window is answered with the oracle's bytes or refused, never answered otherwise."""
    ws = lg.windows("stacked", 11, 3, small=True) + lg.windows("own_ins", 11, 3, small=True)
    b = build_batch(ws)
    off = b.slot_layout()
    want = oracle_lib.poa_batch(b, off=off)[0]
    seen = set()
    for kb in (64, 256, 1024, 2048):
        cons, st, res, _, _ = emu.poa_giant(b, off=off, slice_bytes=kb << 10)
        for i in range(len(ws)):
            assert res[i] in (emu_util.RES_OK, emu_util.RES_OVERFLOW) and (res[i] != emu_util.RES_OK or cons[i] == want[i]), (kb, i)
            seen.add(int(res[i]))
    assert seen == {emu_util.RES_OK, emu_util.RES_OVERFLOW}


def _asan_check():
    """(child process of the test below) stacked and giant windows through class 6 with slices of exactly the size handed over, under
    AddressSanitizer: a table that the second round outgrows is an overrun of the slice here, and a wrong consensus in any case."""
    import oracle
    e = emu_util.Emu(asan=True)
    orc = oracle.Oracle()
    n = 0
    for ws, slice_bytes in ((lg.windows("stacked", 5, 3, small=True), 4 << 20), (lg.windows("giant", 3, 1)[:1], SLICE)):
        b = build_batch(ws)
        off = b.slot_layout()
        cons, st, res, _, _ = e.poa_giant(b, off=off, slice_bytes=slice_bytes)
        assert all(r == emu_util.RES_OK for r in res) and cons == orc.poa_batch(b, off=off)[0]
        n += len(ws)
    return n


def test_stacked_and_giant_under_asan():
    emu_util.build()
    libasan = subprocess.check_output(["gcc", "-print-file-name=libasan.so"], text=True).strip()
    env = dict(os.environ, LD_PRELOAD=libasan, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0")
    here = os.path.dirname(os.path.abspath(__file__))
    code = "import sys; sys.path[:0] = [%r, %r]; import test_long_growth_cpu as t; print('windows', t._asan_check())" % (os.path.dirname(here), here)
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0 and "windows" in p.stdout, (p.stdout[-400:], p.stderr[-1500:])


# ---- the bounded LONG space -----------------------------------------------------------------------------------------------------
# exhaustive_parity.LONG_SPACES["l2n3"]: alphabet {A, C}, drafts of 1-4 bases, 3 arms of 0-4 bases, every kind multiset: 8 937 300
# windows.  Both rounds and curate's floor(0.4 * n_internal) (n_internal 0, 1, 2: threshold 0; 3: 1) where ties are dense.  The real
# reference drops every arm shorter than 19 bases (Filter::is_good finds no minimizer), so this space is pinned to the ORACLE.  The
# emulator takes 1 ms (class 6), 2 ms (class 4) and 45 ms (class 5: it initialises its tables per window) per window, so every K-th
# window of the enumeration runs, K per class below: about 6 000, 3 000 and 300 windows, times two score sets, in about a minute.
# (tests/test_gpu_long_growth.py runs the whole space on the device.)
LONG_SPACE_STRIDE = {6: 1499, 4: 2999, 5: 29989}


@pytest.mark.parametrize("cfg", [6, 4, 5])
def test_bounded_long_space_vs_oracle(emu, oracle_lib, cfg):
    n = 0
    for scores in ex.LONG_SCORE_SETS:
        for b in ex.every_kth("l2n3", LONG_SPACE_STRIDE[cfg]):
            off = b.slot_layout()
            want, wst, _, _ = oracle_lib.poa_batch(b, scores=scores, off=off)
            if cfg == 6:
                cons, st, res, _, _ = emu.poa_giant(b, scores=scores, off=off, slice_bytes=1 << 20)
            else:
                cons, st, res, _, _ = emu.poa_batch(b, cfg, scores=scores, off=off)
            bad = [i for i in range(b.n_windows) if res[i] != emu_util.RES_OK or st[i] != wst[i] or cons[i] != want[i]]
            assert not bad, f"class {cfg} scores {scores}: {ex.describe(b, bad[0])}: result {int(res[bad[0]])} {cons[bad[0]]!r}, oracle {want[bad[0]]!r}"
            n += b.n_windows
    assert n >= 2 * (ex.space_size("l2n3") // LONG_SPACE_STRIDE[cfg])
