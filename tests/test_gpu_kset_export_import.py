"""GPU: hypo_gpu_kset_export / hypo_gpu_kset_import (kset_kernel.hip) against the CPU checker (tests/kset_file_checker.py), as exact
integers, at k = 12, 21, 22 and 31 on sets that count and sets that do not.  The k-mers are those of generated reads of a 2 kbp
genome with errors, a poly-A read and one read 300 times, so that count bytes reach 255.  Export: every cap, the records as a dict
are the model, the n_out add up, the device's digest is the checker's, a second sequence returns the same arrays, nothing is
written beyond n_out.  Import: in pieces of 300 into the smallest table, which grows while counts exist; the set then answers as
the one built from the reads, and as the checker; two half-stream exports give the whole stream's set.  Then what the kernels could
lose a race on, and every refused call, which must leave the set as it was."""
import ctypes as C
import functools

import numpy as np
import pytest

import kset_file_checker as kf
import qv_checker as qc
import qv_track_checker as tc
import test_gpu_kset as tk
from hypo_amd import abi

pytestmark = pytest.mark.gpu
KS = [12, 21, 22, 31]
MIN_SLOTS = 1024
# what the arrays of an export call hold before it (no key has its top bits set, a record's count byte is never 0)
UNTOUCHED64, UNTOUCHED8 = 0xFFFFFFFFFFFFFFFF, 0


@pytest.fixture(scope="module")
def gpu():
    from hypo_amd import capi
    return capi.HypoGpu(0)


@functools.lru_cache(maxsize=None)
def case(k):
    """(records, texts to ask, the model with counts): the repeated read's copies are spread over both halves of the list"""
    rng = np.random.default_rng(4000 + k)
    genome, recs = tk.read_records(rng, k, genome_len=2000, cov=30, read_len=100)
    often = tk.mutate(rng, genome[300:400], 0.03)
    half = len(recs) // 2
    recs = recs[:half] + [often] * 150 + [b"A" * 320] + recs[half:] + [often] * 150
    texts = [genome, tk.mutate(rng, genome, 0.01), often, b"A" * 40, tk.rnd(rng, 500)]
    m = kf.model(recs, k)
    assert max(m.values()) == 255 and sum(1 for c in m.values() if c == 255) > 50 and 1 in m.values() and 2000 < len(m) < 100000
    return recs, texts, m


def model_of(k, counting):
    m = case(k)[2]
    return m if counting else {key: 1 for key in m}


def begin(gpu, k, counting, expected=1, max_bytes=0):
    gpu.kset_begin(k, expected, max_bytes)
    if counting:
        gpu.kset_counts_enable(1)


def slots_of(gpu, counting):
    tb = gpu.kset_size()[1]
    for slots in range(tb // 10 - 64 if counting else tb // 8, tb // 8 + 1):
        if slots * 8 + (2 * ((slots + 255) // 256) * 256 if counting else 0) == tb:
            return slots
    raise AssertionError(tb)


def export_call(gpu, cursor, cap, counts=True, room=None):
    """one call of hypo_gpu_kset_export into fresh arrays of `room` entries (cap when None) that hold the sentinels:
    (return code, cursor after the call, n_out or None when it was not written, keys, counts or None, digest of the call)"""
    room = max(1, cap if room is None else room)
    keys = np.full(room, UNTOUCHED64, np.uint64)
    cnt = np.full(room, UNTOUCHED8, np.uint8) if counts else None
    rc, cur, n, dig = gpu.kset_export_rc(cursor, cap, keys, cnt)
    return rc, cur, n, keys, cnt, dig


def sequence(gpu, cap, counts=True, room=None):
    """one export sequence call by call: (keys, counts, digest, n_outs); nothing beyond n_out is written"""
    cursor, keys, cnts, digest, n_outs = 0, [], [], 0, []
    while cursor != abi.KSET_EXPORT_END:
        rc, cursor, n, k, c, d = export_call(gpu, cursor, cap, counts, room=(cap if room is None else room) + 3)
        assert rc == 0 and n <= cap
        assert (k[n:] == UNTOUCHED64).all() and (c is None or (c[n:] == UNTOUCHED8).all())
        keys.append(k[:n])
        cnts.append(c[:n] if counts else None)
        digest = (digest + d) & kf.M64
        n_outs.append(n)
        assert len(n_outs) < 200000
    return np.concatenate(keys), (np.concatenate(cnts) if counts else None), digest, n_outs


def as_dict(keys, counts):
    d = dict(zip(keys.tolist(), counts.tolist()))
    assert len(d) == keys.size, "a record came twice"
    return d


def answers(gpu, k, texts, counting):
    """what the set says to everyone who asks it"""
    out = {"size": gpu.kset_size()[0], "query": [a.tolist() for a in gpu.kset_query(texts)], "track": [np.asarray(a).tolist() for a in gpu.kset_query_track(texts)]}
    if counting:
        out["spectrum"] = gpu.kset_spectrum(0).tolist()
        for t in (2, 3):
            gpu.kset_min_count(t)
            out["query%d" % t] = [a.tolist() for a in gpu.kset_query(texts)]
        gpu.kset_min_count(1)
    return out


def check_answers(ans, k, texts, m, counting):
    R = np.array(sorted(m), np.uint64)
    assert ans["size"] == len(m)
    assert list(zip(*ans["query"])) == [qc.seq_stats(t, k, R) for t in texts]
    assert ans["track"] == [list(x) for x in tc.track(texts, k, R)]
    if counting:
        hist = np.bincount(np.array(list(m.values())), minlength=256)
        S = np.array(ans["spectrum"])
        assert S[:, 0].tolist() == hist.tolist() and not S[:, 1:].any()
        for t in (2, 3):
            Rt = np.array(sorted(key for key, c in m.items() if c >= t), np.uint64)
            assert list(zip(*ans["query%d" % t])) == [qc.seq_stats(x, k, Rt) for x in texts]


@pytest.mark.parametrize("counting", [False, True])
@pytest.mark.parametrize("k", KS)
def test_export_then_import(gpu, k, counting):
    recs, texts, _ = case(k)
    m = model_of(k, counting)
    begin(gpu, k, counting)
    try:
        for at in range(0, len(recs), 40):                               # (in small adds: the table doubles, and ends no larger than it must)
            gpu.kset_add(b"\n".join(recs[at:at + 40]))
        assert gpu.kset_size()[0] == len(m) and slots_of(gpu, counting) > 4 * MIN_SLOTS        # (it grew)
        first = None
        for cap in (7, 1000, 1 << 20):
            keys, counts, dig, n_outs = sequence(gpu, cap)
            assert as_dict(keys, counts) == m and sum(n_outs) == len(m) == keys.size and dig == kf.digest(m)
            again = sequence(gpu, cap)
            assert np.array_equal(again[0], keys) and np.array_equal(again[1], counts) and again[2:] == (dig, n_outs)
            # the order is that of the table, whatever the cap
            assert first is None or (np.array_equal(first[0], keys) and np.array_equal(first[1], counts))
            first = (keys, counts)
        # without counts: the keys alone, the same digest (the count of a record is what the set holds)
        k2, c2, d2, _ = sequence(gpu, 1000, counts=False)
        assert c2 is None and np.array_equal(k2, keys) and d2 == dig
        # the binding's own loop
        k3, c3, d3, n3 = gpu.kset_export(4096)
        assert np.array_equal(k3, keys) and np.array_equal(c3, counts) and d3 == dig and sum(n3) == keys.size
        src = answers(gpu, k, texts, counting)
        check_answers(src, k, texts, m, counting)
        gpu.kset_end()

        # into the smallest table, in pieces of 300: it grows while counts exist
        begin(gpu, k, counting)
        assert slots_of(gpu, counting) == MIN_SLOTS
        dsum, grew = 0, 0
        for at in range(0, keys.size, 300):
            before = gpu.kset_size()[1]
            dsum = (dsum + gpu.kset_import(keys[at:at + 300], counts[at:at + 300])) & kf.M64
            grew += gpu.kset_size()[1] != before
        assert dsum == dig and grew >= 3
        assert answers(gpu, k, texts, counting) == src
        again = sequence(gpu, 1000)
        assert as_dict(again[0], again[1]) == m and again[2] == dig
    finally:
        gpu.kset_end()


@pytest.mark.parametrize("counting", [False, True])
@pytest.mark.parametrize("k", KS)
def test_cap_of_one_on_the_smallest_table(gpu, k, counting):
    rng = np.random.default_rng(4100 + k)
    recs = [tk.rnd(rng, 300), b"A" * 200]
    m = kf.model(recs, k, counting)
    begin(gpu, k, counting)
    try:
        for r in recs:
            gpu.kset_add(r)
        assert slots_of(gpu, counting) == MIN_SLOTS and gpu.kset_size()[0] == len(m)
        keys, counts, dig, n_outs = sequence(gpu, 1)
        assert len(n_outs) == MIN_SLOTS and set(n_outs) == {0, 1} and sum(n_outs) == len(m)
        assert as_dict(keys, counts) == m and dig == kf.digest(m)
        # a tile that is not full, and a range that ends at the table's end: 1024 = 3 * 300 + 124
        again = sequence(gpu, 300)
        assert np.array_equal(again[0], keys) and np.array_equal(again[1], counts) and again[2] == dig and len(again[3]) == 4
    finally:
        gpu.kset_end()


@pytest.mark.parametrize("counting", [False, True])
@pytest.mark.parametrize("k", KS)
def test_two_halves_give_the_whole(gpu, k, counting):
    recs, _, _ = case(k)
    m = model_of(k, counting)
    half = len(recs) // 2
    parts = []
    try:
        for piece in (recs[:half], recs[half:]):
            begin(gpu, k, counting)
            gpu.kset_add(b"\n".join(piece))
            keys, counts, dig, _ = sequence(gpu, 1 << 20)
            assert as_dict(keys, counts) == kf.model(piece, k, counting)
            parts.append((keys, counts, dig))
            gpu.kset_end()
        if counting:                                                      # the halves saturate nothing the whole does not
            assert sum(1 for c in parts[0][1].tolist() if c == 255) < sum(1 for c in m.values() if c == 255)
        begin(gpu, k, counting)
        for keys, counts, dig in parts:
            assert gpu.kset_import(keys, counts) == dig
        keys, counts, dig, _ = sequence(gpu, 1 << 20)
        assert as_dict(keys, counts) == m and dig == kf.digest(m) and gpu.kset_size()[0] == len(m)
    finally:
        gpu.kset_end()


@pytest.mark.parametrize("k", KS)
def test_races_the_kernels_can_lose(gpu, k):
    # keys no other part of this test uses: the first canonical codes of some home slots of the smallest table
    fresh = iter(kf.same_home(17, MIN_SLOTS, k, 6))
    begin(gpu, k, True)
    try:
        want = {}
        a, b, c, d, e = (next(fresh) for _ in range(5))
        gpu.kset_import([a] * 300)                                       # one call, the same new key 300 times, NULL counts
        want[a] = 255
        gpu.kset_import([b] * 300, [1] * 300)
        want[b] = 255
        gpu.kset_import([c, c], [200, 100])
        want[c] = 255
        gpu.kset_import([d, e, d, e], [250, 250, 5, 4])
        want[d], want[e] = 255, 254
        gpu.kset_import([e], [1])
        want[e] = 255
        gpu.kset_import([e, a], [255, 255])                              # full stays full
        keys, counts, dig, _ = sequence(gpu, 1000)
        assert as_dict(keys, counts) == want and dig == kf.digest(want) and slots_of(gpu, True) == MIN_SLOTS
    finally:
        gpu.kset_end()
    # keys in neighbouring slots: the four count bytes of one 32-bit word are added to in one launch
    begin(gpu, k, True)
    try:
        quad = [kf.same_home(s, MIN_SLOTS, k, 1)[0] for s in range(512, 520)]
        gpu.kset_import(quad * 60, [3] * (60 * len(quad)))
        keys, counts, dig, _ = sequence(gpu, 1024)
        assert keys.tolist() == quad and counts.tolist() == [180] * 8     # every key sits in its home slot, in slot order
        gpu.kset_import(quad[::-1] * 37, ([1, 2] * 4) * 37)
        keys, counts, dig, _ = sequence(gpu, 1024)
        want = {key: 180 + 37 * c for key, c in zip(quad[::-1], [1, 2] * 4)}
        assert sorted(set(want.values())) == [217, 254] and as_dict(keys, counts) == want
        gpu.kset_import(quad * 2)
        keys, counts, dig, _ = sequence(gpu, 1024)
        assert as_dict(keys, counts) == {key: min(255, c + 2) for key, c in want.items()} and 255 in counts.tolist() and 219 in counts.tolist()
    finally:
        gpu.kset_end()


@pytest.mark.parametrize("counting", [False, True])
@pytest.mark.parametrize("k", KS)
def test_probes_wrap_and_export_crosses_the_tables_end(gpu, k, counting):
    """eight keys whose probes start at the last slot: one stays there, seven wrap to slots 0..6"""
    last = kf.same_home(MIN_SLOTS - 1, MIN_SLOTS, k, 8)
    begin(gpu, k, counting)
    try:
        given = {key: i + 1 for i, key in enumerate(last)}
        want = given if counting else {key: 1 for key in last}
        assert gpu.kset_import(last, list(range(1, 9))) == kf.digest(given)          # (the digest of the records as given)
        assert slots_of(gpu, counting) == MIN_SLOTS and gpu.kset_size()[0] == 8
        keys, counts, dig, n_outs = sequence(gpu, 1000)                   # slots [0, 1000), then [1000, 1024)
        assert n_outs == [7, 1] and as_dict(keys, counts) == want and dig == kf.digest(want)
        for cap in (1, 7, 1024):
            again = sequence(gpu, cap)
            assert np.array_equal(again[0], keys) and np.array_equal(again[1], counts) and again[2] == dig
            assert cap != 1 or [i for i, n in enumerate(again[3]) if n] == list(range(7)) + [MIN_SLOTS - 1]
        total, missing = gpu.kset_query([b"A" * 64])                      # (a probe that finds nothing ends)
        assert int(total[0]) == 64 - k + 1
    finally:
        gpu.kset_end()


@pytest.mark.parametrize("counting", [False, True])
@pytest.mark.parametrize("k", KS)
def test_refused_calls_change_nothing(gpu, k, counting):
    rng = np.random.default_rng(4200 + k)
    recs = [tk.rnd(rng, 300)]
    m = kf.model(recs, k, counting)
    err = lambda: gpu.lib.hypo_gpu_last_error().decode()
    begin(gpu, k, counting)
    try:
        gpu.kset_add(recs[0])
        slots = slots_of(gpu, counting)
        before = sequence(gpu, 1000)
        assert as_dict(before[0], before[1]) == m

        def unchanged():
            now = sequence(gpu, 1000)
            return np.array_equal(now[0], before[0]) and np.array_equal(now[1], before[1]) and now[2:] == before[2:] and gpu.kset_size()[0] == len(m)
        # export: cap == 0, cap = 2^32, a cursor at and beyond the table's end
        for cursor, cap in ((0, 0), (0, 1 << 32), (slots, 10), (slots + 5, 10), (1 << 40, 10)):
            rc, cur, n, keys, counts, dig = export_call(gpu, cursor, cap, room=16)
            assert rc == abi.HYPO_E_INVALID and (cur, n, dig) == (cursor, None, 0), (cursor, cap)
            assert (keys == UNTOUCHED64).all() and (counts == UNTOUCHED8).all()
        # a finished sequence stays finished
        rc, cur, n, keys, _, _ = export_call(gpu, abi.KSET_EXPORT_END, 10)
        assert (rc, cur, n) == (0, abi.KSET_EXPORT_END, 0) and (keys == UNTOUCHED64).all()
        assert unchanged()
        # import: a key that is no code of k bases, one that is not canonical, a zero count byte; the message names the index
        good = [key for key in sorted(kf.model([tk.rnd(rng, 200)], k)) if key not in m][:20]
        assert len(good) == 20
        not_canonical = next(kf.revcomp(key, k) for key in good if kf.revcomp(key, k) != key)
        for bad_key, bad_count, word in ((4 ** k, 1, "4^"), ((1 << 63) + 5, 1, "4^"), (not_canonical, 1, "canonical"), (good[7], 0, "count byte")):
            keys = good[:13] + [bad_key] + good[13:]
            counts = [2] * 13 + [bad_count] + [2] * (len(good) - 13)
            rc, dig = gpu.kset_import_rc(keys, counts)
            assert rc == abi.HYPO_E_INVALID and dig == 0 and "record 13" in err() and word in err(), err()
            assert unchanged()
        # the least offending index is the one named, and NULL counts have no zero
        rc, _ = gpu.kset_import_rc([4 ** k] * 500)
        assert rc == abi.HYPO_E_INVALID and "record 0:" in err()
        rc, dig = gpu.kset_import_rc([], [])
        assert (rc, dig) == (0, 0) and unchanged()                        # n == 0 touches nothing
        one = np.array(good[:1], np.uint64)
        assert gpu.lib.hypo_gpu_kset_import(None, None, C.c_uint64(3), None) == abi.HYPO_E_INVALID and unchanged()
        assert gpu.lib.hypo_gpu_kset_import(one.ctypes.data_as(C.c_void_p), None, C.c_uint64(1 << 32), None) == abi.HYPO_E_INVALID and unchanged()
        if counting:                                                      # a closed set takes no records, and exports as before
            gpu.kset_mark(0, [recs[0][:100]])
            rc, dig = gpu.kset_import_rc(good, [1] * len(good))
            assert rc == abi.HYPO_E_INVALID and dig == 0 and "closed" in err()
            assert unchanged()
    finally:
        gpu.kset_end()
    # a cap that allows no growth: HYPO_E_CAPACITY, and the set is what it was
    begin(gpu, k, counting, max_bytes=10 * MIN_SLOTS)                     # (the smallest table with its counts; 1280 slots without)
    try:
        slots = slots_of(gpu, counting)
        assert slots == MIN_SLOTS
        some = sorted(kf.model([tk.rnd(rng, 1000)], k))[:700]
        assert len(some) == 700
        want = {key: 3 if counting else 1 for key in some[:100]}
        assert gpu.kset_import(some[:100], [3] * 100) == kf.digest({key: 3 for key in some[:100]})
        before = sequence(gpu, 1000)
        assert as_dict(before[0], before[1]) == want
        rc, dig = gpu.kset_import_rc(some[100:], [3] * 600)
        assert rc == abi.HYPO_E_CAPACITY and dig == 0 and "--qv-mem" in err()
        now = sequence(gpu, 1000)
        assert np.array_equal(now[0], before[0]) and np.array_equal(now[1], before[1]) and now[2] == before[2] and slots_of(gpu, counting) == slots
    finally:
        gpu.kset_end()
    # no set
    rc, dig = gpu.kset_import_rc([1], [1])
    assert rc == abi.HYPO_E_INVALID and "no k-mer set" in err()
    rc, cur, n, keys, _, _ = export_call(gpu, 0, 10)
    assert rc == abi.HYPO_E_INVALID and (cur, n) == (0, None) and "no k-mer set" in err()
