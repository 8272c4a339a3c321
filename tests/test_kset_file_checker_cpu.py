"""CPU: tests/kset_file_checker.py pinned.  Its canonical codes are qv_checker's, mix64 and the home slot have their known values,
the digest does not depend on the order, a file written and parsed gives its blocks back, every refusal DESIGN asks of a reader
("k-mer set file") is raised for the file made to provoke it, and the merge of two halves of a read stream is the model of the
whole, with saturation."""
import random

import numpy as np
import pytest

import kset_file_checker as kf
import qv_checker as qc


def reads(seed, n=40, length=120):
    rnd = random.Random(seed)
    g = "".join(rnd.choice("ACGT") for _ in range(1500))
    out = []
    for _ in range(n):
        at = rnd.randrange(len(g) - length)
        out.append(g[at:at + length].encode())
    return out + [b"A" * 300, b"ACGTNNACGTACGTACGTACGTACGTACGTACGTAC"]


def test_mix64_and_home():
    # MurmurHash3's fmix64: 0 is a fixed point, and the value of 1 is the published one
    assert kf.mix64(0) == 0
    assert kf.mix64(1) == 0xB456BCFC34C2CB2C
    for key in (1, 12345, (1 << 61) + 7):
        for slots in (1024, 1025, 1 << 33):
            assert 0 <= kf.home(key, slots) < slots
            assert kf.home(key, slots) == (kf.mix64(key) * slots) // (1 << 64)


@pytest.mark.parametrize("k", [12, 21, 22, 31])
def test_canonical_codes_are_qv_checkers(k):
    rnd = random.Random(k)
    for _ in range(50):
        s = "".join(rnd.choice("ACGT") for _ in range(k))
        fwd = 0
        for ch in s:
            fwd = (fwd << 2) | "ACGT".index(ch)
        rc_text = "".join("TGCA"["ACGT".index(ch)] for ch in reversed(s))
        rc = 0
        for ch in rc_text:
            rc = (rc << 2) | "ACGT".index(ch)
        assert kf.revcomp(fwd, k) == rc and kf.revcomp(rc, k) == fwd
        assert kf.canonical(fwd, k) == int(qc.canonical_windows(s.encode(), k)[0]) == kf.canonical(rc, k)


def test_model_is_the_read_set_with_counts():
    k = 21
    rs = reads(3)
    m = kf.model(rs, k)
    assert sorted(m) == qc.read_set(rs, k).tolist()
    assert m[0] == 255                                                  # poly-A: 280 windows of one key
    w = np.concatenate([qc.canonical_windows(r, k) for r in rs])
    for key in list(m)[:200]:
        assert m[key] == min(255, int(np.count_nonzero(w == key)))
    assert set(kf.model(rs, k, counting=False).values()) == {1}


def test_digest_does_not_depend_on_order():
    m = kf.model(reads(5), 21)
    recs = list(m.items())
    d = kf.digest(recs)
    random.Random(1).shuffle(recs)
    assert kf.digest(recs) == d == kf.digest(m)
    assert kf.digest(recs[:-1]) != d and kf.digest([]) == 0
    key, c = recs[0]
    assert kf.record_digest(key, c) == (kf.mix64(key) + c * kf.GOLD) % (1 << 64)
    assert kf.digest([(key, c + 1)] + recs[1:]) != d


def blocks_of(m, sizes):
    recs, out, at = sorted(m.items()), [], 0
    for s in sizes:
        out.append(recs[at:at + s])
        at += s
    out.append(recs[at:])
    return [b for b in out if b]


def test_round_trip(tmp_path):
    m = kf.model(reads(7), 22)
    blocks = blocks_of(m, [5, 8, 1, 300])
    p = str(tmp_path / "s.hks")
    kf.write_file(p, 22, blocks)
    k, n_keys, got, dig = kf.parse_file(p)
    assert (k, n_keys, got, dig) == (22, len(m), blocks, kf.digest(m))
    data = open(p, "rb").read()
    assert len(data) == 24 + sum(8 + 8 * len(b) + (len(b) + 7) // 8 * 8 for b in blocks) + 16
    assert data[:8] == b"HYPOKSET" and data[8:24] == (1).to_bytes(4, "little") + (22).to_bytes(4, "little") + len(m).to_bytes(8, "little")
    # an empty set: a header and the end
    assert kf.parse_bytes(kf.file_bytes(21, [])) == (21, 0, [], 0)


def test_every_refusal():
    m = kf.model(reads(9), 21)
    blocks = blocks_of(m, [5, 11])
    bad = kf.corrupted(21, blocks)
    assert {kf.cause_of(n) for n in bad} == set(kf.CAUSES)
    for name, data in bad.items():
        with pytest.raises(kf.BadFile) as e:
            kf.parse_bytes(data)
        assert str(e.value) == kf.cause_of(name), name
    kf.parse_bytes(kf.file_bytes(21, blocks))


def test_merge_of_two_halves_is_the_whole():
    k = 21
    rs = reads(11) + [reads(11)[0]] * 300                              # one read 301 times: its keys pass 255 only in the whole
    half = len(rs) // 2 + 30
    a, b, whole = kf.model(rs[:half], k), kf.model(rs[half:], k), kf.model(rs, k)
    assert kf.merge(a, b) == whole == kf.merge(b, a)
    assert any(a.get(key, 0) < 255 and b.get(key, 0) < 255 and c == 255 for key, c in whole.items())
    assert kf.merge({5: 250}, {5: 5}) == {5: 255} and kf.merge({5: 250}, {5: 4}) == {5: 254} and kf.merge({5: 200}, {5: 100}) == {5: 255}


def test_same_home():
    for k, slots in ((12, 1024), (31, 1024)):
        keys = kf.same_home(slots - 1, slots, k, 8)
        assert len(set(keys)) == 8 and all(kf.home(x, slots) == slots - 1 and x <= kf.revcomp(x, k) and x < 4 ** k for x in keys)
