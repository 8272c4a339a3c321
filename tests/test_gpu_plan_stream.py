"""GPU: the plan kernel's arm comparison (poa_plan_count_kernel: eight bytes of four arm pairs per step, the last word of an arm
loaded so that it ends with the arm) and the stream assignment of the first passes (PoaSchedule::main_class, HYPO_POA_MAIN; side
streams forked and joined only when they run something).  Batches at which the plan takes another path: one window, a ragged last
workgroup, arm ranges beyond the staged lengths, arms of fewer than four, fewer than eight and of more packed bytes, trivial next to
LONG windows, descriptors whose arms run past the arm table.  (The kernel is not persistent: no batch for a looping workgroup.)
Consensus against the oracle; the class counts against what the commit before this kernel produced on an MI355X for the same
batches (PARENT_STATS: recorded from a run of that commit; the plan's keys decide n_class / n_escalated / n_trivial)."""
import numpy as np
import pytest

from hypo_amd import abi, capi, sim
from hypo_amd.batch import HostBatch

pytestmark = pytest.mark.gpu


def _tiny(n, seed):
    """n windows of 8 - 20 bases with 3 - 8 internal arms: class 0 almost only (the dense shape: four groups per wave)"""
    rng = np.random.default_rng(seed)
    z = np.zeros(n, np.int64)
    return np.stack([rng.integers(8, 21, size=n), rng.integers(3, 9, size=n), z, z, z], axis=1)


def _many_arms():
    """200 SHORT windows of about 200 arms: the 64 windows of a round span ~12 800 arms, beyond the staged range."""
    rng = np.random.default_rng(210)
    n = 200
    shapes = np.stack([rng.integers(40, 56, size=n), rng.integers(188, 204, size=n), rng.integers(0, 6, size=n),
                       rng.integers(0, 6, size=n), np.zeros(n, np.int64)], axis=1)
    return sim.window_batch(0, seed=211, shapes=shapes)


def _trivial_and_long():
    """Trivial windows (fewer than two arms; more empty arms than arms) between C1-shaped ones, and a few LONG windows."""
    rng = np.random.default_rng(310)
    tab, cnt = sim.load_shape("c1_shape")
    plain = tab[rng.choice(tab.shape[0], size=120, p=cnt / cnt.sum())]
    z = np.zeros(40, np.int64)
    no_arm = np.stack([rng.integers(20, 90, size=40), z, z, z, z], axis=1)
    one_arm = np.stack([rng.integers(20, 90, size=40), z + 1, z, z, z], axis=1)
    empties = np.stack([rng.integers(20, 90, size=40), z + 3, z + 1, z + 1, z + 9], axis=1)
    z6 = np.zeros(6, np.int64)
    longs = np.stack([rng.integers(120, 500, size=6), rng.integers(12, 45, size=6), z6, z6, rng.integers(0, 3, size=6)], axis=1)
    shapes = np.concatenate([plain, no_arm, one_arm, empties, longs])
    mask = np.concatenate([np.zeros(240, bool), np.ones(6, bool)])
    perm = rng.permutation(shapes.shape[0])
    return sim.window_batch(0, seed=311, shapes=shapes[perm], long_mask=mask[perm])


PAST_TABLE = (5, 70, 200)                 # windows of the "past_table" batch whose descriptors are bent


def _past_table():
    """300 C1-shaped windows; three descriptors whose arms run past the arm table: from the last arm on, from one past the end, and
    with a count that wraps 32 bits.  Returns the batch as the device gets it and the intact one (for the oracle)."""
    b = sim.window_batch(300, seed=33)
    w = b.windows.copy()
    for i in PAST_TABLE:
        assert int(w["n_internal"][i]) >= 2
    w["first_arm"][PAST_TABLE[0]] = b.n_arms - 1
    w["first_arm"][PAST_TABLE[1]] = b.n_arms
    w["n_internal"][PAST_TABLE[2]] = 0xfffffff0
    return HostBatch(w, b.draft4, b.arm_off, b.arm_len, b.arms2), b


BATCHES = {
    "one_window": lambda: sim.window_batch(1, seed=78),
    "ragged_193": lambda: sim.window_batch(193, seed=194),
    "c1_4000": lambda: sim.window_batch(4000, seed=78),
    "many_arms": _many_arms,
    "trivial_and_long": _trivial_and_long,
}

# stats() of the parent commit, on an MI355X, for BATCHES and the "past_table" batch
PARENT_STATS = {
    'one_window': {'n_class': [1, 0, 0, 0, 0, 0, 0, 0], 'n_escalated': 0, 'n_trivial': 0, 'n_failed': 0},
    'ragged_193': {'n_class': [121, 37, 35, 0, 0, 0, 0, 0], 'n_escalated': 0, 'n_trivial': 0, 'n_failed': 0},
    'c1_4000': {'n_class': [2512, 822, 666, 0, 0, 0, 0, 0], 'n_escalated': 0, 'n_trivial': 0, 'n_failed': 0},
    'many_arms': {'n_class': [0, 0, 0, 2, 198, 0, 0, 0], 'n_escalated': 0, 'n_trivial': 0, 'n_failed': 0},
    'trivial_and_long': {'n_class': [108, 78, 54, 0, 6, 0, 0, 0], 'n_escalated': 0, 'n_trivial': 120, 'n_failed': 0},
    'past_table': {'n_class': [198, 60, 39, 0, 0, 0, 0, 0], 'n_escalated': 0, 'n_trivial': 3, 'n_failed': 3},
}

STAT_FIELDS = ("n_class", "n_escalated", "n_trivial", "n_failed")


@pytest.fixture(scope="module")
def gpu():
    return capi.HypoGpu(0)


def _same_as_oracle(db, expect, off, skip=()):
    bases, _, ln, st = db.results()
    ob, oln, ost = expect
    for i in skip:
        assert st[i] == abi.ST_INVALID and ln[i] == 0, (i, st[i])
    keep = np.ones(len(ln), bool)
    keep[list(skip)] = False
    assert (st[keep] == ost[keep]).all() and (ln[keep] == oln[keep]).all()
    for i in np.flatnonzero(keep):
        o, l = int(off[i]), int(ln[i])
        assert (bases[o:o + l] == ob[o:o + l]).all(), i


def _oracle(oracle_lib, b, off):
    ob, _, oln, ost, _, _ = oracle_lib.poa_batch_raw(b, off=off)
    return ob, oln, ost


def _check_stats(name, db):
    stats = db.stats()
    got = {f: stats[f] for f in STAT_FIELDS}
    print("PARENT_STATS", repr(name), got)
    assert got == PARENT_STATS[name]


@pytest.mark.parametrize("name", list(BATCHES))
def test_plan_batches(gpu, oracle_lib, name):
    b = BATCHES[name]()
    off = b.slot_layout()
    db = gpu.device_batch(b, off=off)
    db.run()
    _same_as_oracle(db, _oracle(oracle_lib, b, off), off)
    _check_stats(name, db)


def test_descriptors_past_the_arm_table(gpu, oracle_lib):
    bad, good = _past_table()
    off = good.slot_layout()
    db = gpu.device_batch(bad, off=off)
    db.run()
    _same_as_oracle(db, _oracle(oracle_lib, good, off), off, skip=PAST_TABLE)
    _check_stats("past_table", db)


def test_stream_sequence(oracle_lib, monkeypatch):
    """One context through every stream assignment: history picks the caller's-stream class (mixed, dense, class-2 heavy batches), a
    LONG first pass on the third side stream, a polling launch on the third and on the fourth, and HYPO_POA_MAIN forcing each class."""
    for k in ("MAIN", "POLL_WAVES"):
        monkeypatch.delenv("HYPO_POA_" + k, raising=False)
    gpu = capi.HypoGpu(0)
    rng = np.random.default_rng(500)
    z = np.zeros(1500, np.int64)
    wide = np.stack([rng.integers(100, 113, size=1500), rng.integers(10, 21, size=1500), z, z, z], axis=1)
    made = {
        "c1": sim.window_batch(4000, seed=79),
        "dense": sim.window_batch(0, seed=501, shapes=_tiny(4000, 502)),
        "wide": sim.window_batch(0, seed=503, shapes=wide),
        "long": sim.c4_batch(0, 12, seed=6),
        "noisy": sim.window_batch(4000, seed=80, read_sub=0.01),
    }
    ready = {}
    for name, b in made.items():
        off = b.slot_layout()
        ready[name] = (gpu.device_batch(b, off=off), _oracle(oracle_lib, b, off), off)

    def run(name, times=1):
        db, expect, off = ready[name]
        for _ in range(times):
            db.run()
            _same_as_oracle(db, expect, off)
        return db.stats()

    run("c1", 3)
    dense = run("dense", 2)
    assert dense["n_class"][0] * 100 >= 85 * 4000            # (what makes the schedule pick four groups per wave)
    wide_stats = run("wide", 2)
    assert wide_stats["n_class"][2] > 750                     # class 2 dominant
    run("long", 2)                                            # the second call goes by the first one's plan: LONG first pass on the third side stream
    monkeypatch.setenv("HYPO_POA_POLL_WAVES", "8")
    run("long")                                               # ... and a polling launch next to it, on the fourth
    monkeypatch.delenv("HYPO_POA_POLL_WAVES")
    run("noisy", 2)                                           # re-queued windows: the second call has a polling launch of its own
    for main in "012":
        monkeypatch.setenv("HYPO_POA_MAIN", main)
        run("c1")
