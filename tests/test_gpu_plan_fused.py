"""GPU: the plan of a POA call (poa_plan_count_kernel with the per-class scan in its last workgroup, then the scatter) on the
batch shapes at which it takes another path: one workgroup, a ragged last workgroup, arm ranges beyond the staged lengths,
trivial windows next to LONG ones, and a context whose first call waits for the counts the kernel wrote to pinned memory.
Consensus against the oracle; the class counts against what the commit before the fused plan produced on an MI355X for the
same batches (PARENT_STATS: recorded from a run of that commit, the plan's keys decide n_class / n_escalated / n_trivial)."""
import numpy as np
import pytest

from hypo_amd import capi, sim

pytestmark = pytest.mark.gpu


def _many_arms():
    """200 SHORT windows of about 200 arms: the 64 windows of a plan workgroup span ~12 800 arms, beyond the staged range."""
    rng = np.random.default_rng(200)
    n = 200
    shapes = np.stack([rng.integers(40, 56, size=n), rng.integers(188, 204, size=n), rng.integers(0, 6, size=n),
                       rng.integers(0, 6, size=n), np.zeros(n, np.int64)], axis=1)
    return sim.window_batch(0, seed=201, shapes=shapes)


def _trivial_and_long():
    """Trivial windows (fewer than two arms; more empty arms than arms) between C1-shaped ones, and a few LONG windows."""
    rng = np.random.default_rng(300)
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
    return sim.window_batch(0, seed=301, shapes=shapes[perm], long_mask=mask[perm])


BATCHES = {
    "c1_4000": lambda: sim.window_batch(4000, seed=77),
    "one_window": lambda: sim.window_batch(1, seed=77),
    "ragged_193": lambda: sim.window_batch(193, seed=193),
    "many_arms": _many_arms,
    "trivial_and_long": _trivial_and_long,
    "long_first_call": lambda: sim.c4_batch(0, 12, seed=5),
}

# stats() of the commit before the fused plan, on an MI355X, for BATCHES (tests' own inputs: seeds above)
PARENT_STATS = {
    'c1_4000': {'n_class': [2480, 864, 656, 0, 0, 0, 0, 0], 'n_escalated': 0, 'n_trivial': 1, 'n_failed': 0},
    'one_window': {'n_class': [0, 1, 0, 0, 0, 0, 0, 0], 'n_escalated': 0, 'n_trivial': 0, 'n_failed': 0},
    'ragged_193': {'n_class': [134, 33, 26, 0, 0, 0, 0, 0], 'n_escalated': 0, 'n_trivial': 0, 'n_failed': 0},
    'many_arms': {'n_class': [0, 0, 0, 7, 193, 0, 0, 0], 'n_escalated': 0, 'n_trivial': 0, 'n_failed': 0},
    'trivial_and_long': {'n_class': [110, 86, 44, 0, 6, 0, 0, 0], 'n_escalated': 0, 'n_trivial': 120, 'n_failed': 0},
    'long_first_call': {'n_class': [0, 0, 0, 0, 12, 0, 0, 0], 'n_escalated': 0, 'n_trivial': 0, 'n_failed': 0},
}

STAT_FIELDS = ("n_class", "n_escalated", "n_trivial", "n_failed")


@pytest.fixture(scope="module")
def gpu():
    return capi.HypoGpu(0)


def _check(gpu, oracle_lib, name, b):
    off = b.slot_layout()
    db = gpu.device_batch(b, off=off)
    db.run()
    bases, _, ln, st = db.results()
    ob, _, oln, ost, _, _ = oracle_lib.poa_batch_raw(b, off=off)
    assert (st == ost).all() and (ln == oln).all()
    for o, l in zip(off[:-1], ln):
        assert (bases[int(o):int(o) + int(l)] == ob[int(o):int(o) + int(l)]).all()
    stats = db.stats()
    got = {f: stats[f] for f in STAT_FIELDS}
    print(name, got)
    assert got == PARENT_STATS[name]


@pytest.mark.parametrize("name", [n for n in BATCHES if n != "long_first_call"])
def test_plan_batches(gpu, oracle_lib, name):
    _check(gpu, oracle_lib, name, BATCHES[name]())


def test_first_call_of_a_context_is_the_long_batch(oracle_lib):
    # a fresh context has no plan history: the call waits for its own plan and sizes the LONG class from the pinned counts
    _check(capi.HypoGpu(0), oracle_lib, "long_first_call", BATCHES["long_first_call"]())
