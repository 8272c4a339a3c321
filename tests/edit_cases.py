"""Hand-built inputs of hypo_gpu_edit_scripts (edit_kernel.hip): named lists of pairs whose distances and bands are controlled, not hoped
for, and per case the condition that makes it worth running — a predicate over the traces of tests/edit_band_model.py, computed from the
inputs alone and never from the device.  Three ingredients:
  homo(n, m)        A^n against C^m: distance max(n, m), every cell a tie;
  block(h, ...)     P^h + S against S + Q^h (a deletion run, then an insertion run: the path runs along diagonal -h) and the mirror
                    S + P^h against Q^h + S (along +h), S random text longer than 2h, P and Q letters S does not hold;
  subs(s, k)        k spaced substitutions in random text.
Every pair ends in two different bytes unless its case is about the suffix, so that the trim leaves the shape alone."""
import functools
import random

import edit_band_model as bm
import edit_checker as ec


def text(seed, n, alpha=b"ACGT"):
    r = random.Random(seed)
    return bytes(r.choice(alpha) for _ in range(n))


def homo(n, m):
    return b"A" * n, b"C" * m


def block(h, s_len, seed, plus=False, alpha=b"AC"):
    """minus (default): G^h + S against S + T^h; plus: S + G^h against T^h + S"""
    S = text(seed, s_len, alpha)
    return (S + b"G" * h, b"T" * h + S) if plus else (b"G" * h + S, S + b"T" * h)


def subs(s, k, last=True):
    """k substitutions spread evenly over s (the last one on the last byte), each to an N, which matches nothing: the distance is k"""
    s = bytearray(s)
    for i in range(k):
        at = len(s) - 1 - (i * len(s)) // k if last else (i * len(s)) // k
        s[at] = 78
    return bytes(s)


def swap(pairs):
    return [(b, a) for a, b in pairs]


def end_differently(a, b):
    """last bytes A / C"""
    return a[:-1] + b"A", b[:-1] + b"C"


# ---- the cases --------------------------------------------------------------------------------------------------------------------

def _fast_band_edges():
    pairs = []
    for h in (62, 63, 64, 65):
        pairs += [block(h, 2 * h + 30, 100 + h), block(h, 2 * h + 30, 200 + h, plus=True)]
        # |m - n| = 1 (odd: the band has the same room on both sides), the same four excursions
        a, b = block(h, 2 * h + 30, 300 + h)
        pairs += [(a, b + b"T"), (b"G" + a, b)]
        a, b = block(h, 2 * h + 30, 400 + h, plus=True)
        pairs += [(a, b"T" + b), (a + b"G", b)]
    pairs += [homo(k, k) for k in (126, 127, 128, 129)]
    # the path on the main diagonal and the distance alone at the edge: k substitutions, |m - n| = 0 and 1
    x = text(99, 254)
    pairs += [(x, subs(x, k)) for k in (127, 128)]
    pairs += [(x, b"N" + subs(x, k)) for k in (127, 129)] + [(b"N" + x, subs(x, k)) for k in (127, 129)]
    return pairs


def _exact_sides(tr):
    """(lo_req - K0, hi_req - (K0 + band - 1), exact) of the fast pass"""
    p = tr["passes"][0]
    return p["lo_req"] - p["lo"], p["hi_req"] - p["hi"], p["exact"]


def _fast_band_edges_condition(pairs, want, traces):
    sides = [_exact_sides(t) for t in traces]
    assert all(t["passes"][0]["kind"] == "fast" and t["passes"][0]["lds"] for t in traces)
    # each bound decides alone, on its last value that passes and on its first that fails
    assert any(lo == 0 and hi <= 0 and ex for lo, hi, ex in sides) and any(lo == -1 and hi <= 0 and not ex for lo, hi, ex in sides)
    assert any(hi == 0 and lo >= 0 and ex for lo, hi, ex in sides) and any(hi == 1 and not ex for lo, hi, ex in sides)
    for i, h in enumerate((62, 63, 64, 65)):
        for q in range(2):
            t, (d, _) = traces[6 * i + q], want[6 * i + q]
            assert d == 2 * h and t["route"] == ("lds" if h <= 63 else "lds+wide"), (h, q, d, t["route"])
    # the band [-63, 64] is not symmetric: at h = 64 the deletion-first pair runs outside it and the wide pass gets a bound above the
    # distance, the insertion-first pair runs on its last diagonal, is found, and still fails the test on the other side
    minus, plus = traces[12], traces[13]
    assert minus["passes"][0]["d_b"] > 128 and minus["passes"][1]["W"] == minus["passes"][0]["d_b"] + 1
    assert plus["passes"][0]["d_b"] == 128 and plus["passes"][1]["W"] == 129
    # h = 63 touches the band's first diagonal (lane 0) in one order and K0 + 126 in the other
    assert _exact_sides(traces[6])[0] == 0 and traces[7]["passes"][0]["hi"] - 63 == 1
    assert [w[0] for w in want[-6:]] == [127, 128, 128, 130, 128, 130] and [t["route"] for t in traces[-6:]] == ["lds", "lds+wide"] * 3
    assert [_exact_sides(t) for t in traces[-6:]] == [(0, -1, True), (-1, 0, False), (0, 0, True), (-1, 1, False), (0, 0, True), (-1, 1, False)]
    homo_t = traces[-10:-6]
    assert [t["route"] for t in homo_t] == ["lds", "lds", "lds+wide", "lds+wide"] and [t["passes"][-1]["W"] for t in homo_t[2:]] == [129, 129]


def _delta_edges():
    pairs = []
    for k in (126, 127, 128, 129):
        s = text(500 + k, 150)
        a, b = s + b"A", s[:70] + b"N" * k + s[70:] + b"C"
        pairs += [(a, b), (b, a)]
    return pairs


def _delta_edges_condition(pairs, want, traces):
    for i, k in enumerate((126, 127, 128, 129)):
        for q in range(2):
            t, (d, _) = traces[2 * i + q], want[2 * i + q]
            p = t["passes"][0]
            assert d == k + 1 and abs(t["m"] - t["n"]) == k
            if k <= 127:
                assert t["route"] == "lds" and p["exact"] and (p["lo_req"], p["hi_req"]) == ((0, k) if q == 0 else (-k, 0))
                if k == 127:                              # both corners on the band's two ends
                    assert (p["lo"], p["hi"]) == ((0, 127) if q == 0 else (-127, 0))
            else:
                assert t["route"] == "probe" and p["W"] == k + 129 and p["bound"] == k + 128 and p["exact"]


def _k0_clamps():
    pairs = []
    for i, (n, m) in enumerate([(1, 1), (1, 127), (127, 1), (1, 128), (128, 1), (2, 129), (3, 130), (130, 3), (64, 64), (63, 65), (100, 120), (30, 40), (63, 63), (64, 62), (62, 64)]):
        pairs.append(end_differently(text(600 + i, n, b"AC"), text(650 + i, m, b"AC")))
    return pairs


def _k0_clamps_condition(pairs, want, traces):
    """The first clamp moves K0 exactly when n + m < 127 (then the band also ends beyond m: "both at once"); the second branch is
    entered only with n + m = 126 and then max(-n, m - 127) is the value K0 already has (README_edits.md), so `K0 == m - 127`
    occurs where the centred band ends on m by itself."""
    kinds = set()
    for t in traces:
        n, m = t["n"], t["m"]
        assert t["sfx"] == 0 and t["passes"][0]["kind"] == "fast"
        K0 = t["passes"][0]["K0"]
        free = min(0, m - n) - (127 - abs(m - n)) // 2
        lo_c, hi_c = free < -n, free >= -n and free + 127 > m
        assert K0 == (-n if lo_c else max(-n, m - 127) if hi_c else free)
        kinds.add("first" if lo_c else "second" if hi_c else "none")
        if lo_c:
            assert n + m < 128 and K0 + 127 > m
        if K0 == m - 127:
            kinds.add("ends on m")
        if K0 == -n:
            kinds.add("starts on -n")
    assert kinds == {"first", "second", "none", "ends on m", "starts on -n"}, kinds


def _lds_edge():
    pairs = []
    for tot in (509, 510, 511, 512):
        n = tot // 2 + 1
        m = tot - n
        x = text(700 + tot, n)
        y = subs(x[:100] + x[100 + n - m:], 3)
        pairs += [(x, y), homo(n, m)]
    z = text(777, 800)
    a, b = end_differently(text(778, 256), text(778, 254))
    pairs.append((a + z, subs(b, 2, last=False)[:-1] + b"C" + z))
    return pairs


def _lds_edge_condition(pairs, want, traces):
    for i, tot in enumerate((509, 510, 511, 512)):
        lowdiv, hp = traces[2 * i], traces[2 * i + 1]
        assert lowdiv["n"] + lowdiv["m"] == tot == hp["n"] + hp["m"]
        assert lowdiv["route"] == ("lds" if tot <= 510 else "long") and hp["route"] == ("lds+wide" if tot <= 510 else "long+wide")
    t = traces[-1]
    assert len(pairs[-1][0]) + len(pairs[-1][1]) > 2000 and t["sfx"] == 800 and t["n"] + t["m"] == 510 and t["route"] == "lds"


SUFFIXES = (0, 1, 63, 64, 65, 127, 128, 129)


def _suffix():
    pairs = []
    for s in SUFFIXES:
        z = text(800 + s, s)
        pairs.append((b"ACGTACG" + z, b"ACTTAC" + b"T" + z))            # a small difference in front
        pairs.append((z, b"GATTC" + z))                                  # the suffix is all of a
        pairs.append((b"GATTC" + z, z))                                  # ... all of b
    y = text(899, 128)
    pairs += [(y[:64], y[:64]), (y, y), (b"", b""), (b"", y[:30]), (y[:30], b"")]
    return pairs


def _suffix_condition(pairs, want, traces):
    for i, s in enumerate(SUFFIXES):
        front, all_a, all_b = traces[3 * i:3 * i + 3]
        assert front["sfx"] == s and front["route"] == "lds" and front["runs"] == len(ec.runs(want[3 * i][1]))
        assert all_a["sfx"] == s == len(pairs[3 * i + 1][0]) and all_a["route"] == "trivial" and ec.cigar(want[3 * i + 1][1]) == "5I" + (f"{s}=" if s else "")
        assert all_b["sfx"] == s and all_b["route"] == "trivial" and ec.cigar(want[3 * i + 2][1]) == "5D" + (f"{s}=" if s else "")
    assert [t["route"] for t in traces[-5:]] == ["trivial"] * 5 and [t["sfx"] for t in traces[-5:]] == [64, 128, 0, 0, 0]
    assert [ec.cigar(w[1]) for w in want[-5:]] == ["64=", "128=", "", "30I", "30D"]


WIDE_HOMO = [(510, 510), (511, 510), (512, 512), (513, 512), (254, 254), (256, 256), (382, 382), (384, 384), (1022, 1022), (1024, 1024)]
WIDE_BLOCK_H = (127, 128, 255, 256, 257)


def _wide_shapes():
    pairs = [homo(n, m) for n, m in WIDE_HOMO]
    for h in WIDE_BLOCK_H:
        pairs += [block(h, 2 * h + 30, 900 + h, alpha=b"ACGT"[:2]), block(h, 2 * h + 30, 950 + h, plus=True)]
    # unrelated text over two letters: up / left ties all along the path, which the homopolymer pairs (all diagonal) do not have
    pairs += [end_differently(text(990, 700, b"AC"), text(991, 700, b"AC")), end_differently(text(992, 500, b"AC"), text(993, 700, b"AC")),
              end_differently(text(994, 700, b"AC"), text(995, 500, b"AC"))]
    return pairs


def _wide_shapes_condition(pairs, want, traces):
    last = [t["passes"][-1] for t in traces]
    assert all(p["kind"] == "wide" and p["vals_lds"] for p in last[:-3])
    assert [t["route"] for t in traces[-3:]] == ["long+wide", "probe", "probe"]
    assert all("D" in w[1] and "I" in w[1] and "X" in w[1] for w in want[-3:])
    assert [(p["W"], p["S"], p["C"]) for p in last[:4]] == [(511, 256, 1), (512, 256, 1), (513, 257, 2), (514, 257, 2)]
    assert all(t["route"] == "long+wide" for t in traces[:4])
    # S either side of a multiple of 64: G steps
    assert [(p["S"], p["G"]) for p in last[4:10]] == [(128, 2), (129, 3), (192, 3), (193, 4), (512, 8), (513, 9)]
    assert {2, 3, 4, 5, 8, 9} <= {p["G"] for p in last} and {1, 2} <= {p["C"] for p in last}
    assert any(p["dropped"] > 0 for p in last) and any(p["dropped"] == 0 for p in last)
    for i, h in enumerate(WIDE_BLOCK_H):
        for q in range(2):
            t, (d, _) = traces[10 + 2 * i + q], want[10 + 2 * i + q]
            assert d == 2 * h and t["route"] == "long+wide" and t["passes"][0]["d_b"] > d + 20, (h, q, d, t["passes"][0]["d_b"])


def _wide_values_edge():
    S = text(1000, 4300)
    return [homo(8191, 8192), homo(8192, 8192), (b"N" * 4200 + S, S + b"R" * 4200)]


def _wide_values_edge_condition(pairs, want, traces):
    last = [t["passes"][-1] for t in traces]
    assert [(p["W"], p["vals_lds"], p["vals_bytes"]) for p in last[:2]] == [(8192, True, 0), (8193, False, 4 * 8193)]
    assert last[2]["W"] > 8192 and not last[2]["vals_lds"] and all(t["route"] == "long+wide" for t in traces)
    assert len(set(want[2][1])) >= 3                       # not all-tie input: matches, a deletion run and an insertion run


PROBE_DELTAS = (128, 200)
PROBE_SUBS = (126, 127, 128, 129, 130, 131)
PROBE_H = (63, 64, 65)


def _probe_edges():
    pairs = []
    for D in PROBE_DELTAS:
        one = []
        for k in PROBE_SUBS:
            x = text(1100 + D + k, 600)
            y = subs(x, k)
            one.append((x, y[:300] + b"N" * D + y[300:]))
        for h in PROBE_H:
            x = text(1200 + D + h, 400, b"AC")
            one.append((b"G" * h + x + b"A", x[:200] + b"N" * D + x[200:] + b"T" * h + b"C"))        # to -h, the far side from D
            one.append((x + b"G" * h + b"A", b"T" * h + x[:200] + b"N" * D + x[200:] + b"C"))        # to D + h
        pairs += one + swap(one)
    return pairs


def _probe_edges_condition(pairs, want, traces):
    per = len(PROBE_SUBS) + 2 * len(PROBE_H)
    seen = set()
    for i, t in enumerate(traces):
        D = PROBE_DELTAS[i // (2 * per)]
        q = i % per
        d = want[i][0]
        assert abs(t["m"] - t["n"]) == D and t["passes"][0]["kind"] == "probe" and t["passes"][0]["W"] == D + 129
        if q < len(PROBE_SUBS):
            assert d == D + PROBE_SUBS[q]
        else:
            assert d == D + 2 * PROBE_H[(q - len(PROBE_SUBS)) // 2] + 1
        assert t["route"] == ("probe" if d <= D + 129 else "probe+second"), (i, d, D, t["route"])
        if t["route"] == "probe+second":
            assert t["passes"][1]["bound"] == t["passes"][0]["d_b"] and t["passes"][1]["W"] == D + 2 * ((t["passes"][0]["d_b"] - D) // 2) + 1
        seen.add(((d - D) // 2, t["route"], t["m"] > t["n"]))
    for sign in (True, False):
        assert (64, "probe", sign) in seen and (65, "probe+second", sign) in seen


def _alternating(k):
    """C A against G A: 1X 1= per unit, and a last X"""
    return b"CA" * k + b"C", b"GA" * k + b"G"


def _gapped(pad):
    """62 x (1= 1D), 62 x (1= 1I), 3 x (1= 1X) behind a common prefix of `pad` bytes: distance 127 on the diagonals [-62, 0], which the
    fast band decides, and 254 runs of one byte each (but the first).  The matched letters change from unit to unit, so that staying
    on one diagonal costs more than the gaps.  A run that is not '=' costs at least 1 and '=' runs lie between them: a pair the fast
    band decides has at most 2 x 127 runs, and one more for its suffix."""
    a1 = b"".join((b"A" if i % 2 == 0 else b"C") + b"G" for i in range(62))
    b1 = a1.replace(b"G", b"")
    a2 = b"".join(b"K" if i % 2 == 0 else b"M" for i in range(62))
    b2 = a2.replace(b"K", b"KR").replace(b"M", b"MR")
    return b"E" * pad + a1 + b"ZZ" + a2 + b"TYTYTY", b"E" * pad + b1 + b"ZZ" + b2 + b"TWTWTW"     # (ZZ: no 2X for the D and I it parts)


def _run_area():
    z = text(1300, 40)
    pairs = [_gapped(61), _gapped(62)]                             # n + m = 510: the LDS form up to its last word; 512: the long form
    pairs += swap(pairs)
    pairs += [(a + z, b + z) for a, b in pairs[:2]]              # a suffix run in front of the runs
    pairs += [_alternating(127), _alternating(128)]                # d = 128 (LDS form, then wide), d = 129 (long, then wide)
    pairs += [(a + z, b + z) for a, b in pairs[6:8]]
    pairs += [(b"AG" * 170, b"A" * 170), (b"A" * 170, b"AG" * 170), (b"AG" * 170 + z, b"A" * 170 + z)]       # 170 x (1= 1D): the wide form alone
    pairs += [homo(200, 131), homo(131, 200), homo(255, 255)]
    return pairs


def _run_area_condition(pairs, want, traces):
    assert [t["n"] + t["m"] for t in traces[:6]] == [510, 512] * 3 and [t["route"] for t in traces[:6]] == ["lds", "long"] * 3
    assert [t["sfx"] for t in traces[:6]] == [0, 0, 0, 0, 40, 40]
    for i, (t, (d, ops)) in enumerate(zip(traces[:6], want[:6])):
        # the most a pair of the fast path can have (see _gapped); with the suffix run that is (n + m) / 2 of the LDS form
        assert d == 127 and t["runs"] == 2 * d + (t["sfx"] > 0) and ops.count("D") == 62 == ops.count("I") and ops.count("X") == 3
    assert traces[4]["runs"] >= (traces[4]["n"] + traces[4]["m"]) // 2
    assert [t["route"] for t in traces[6:10]] == ["lds+wide", "long+wide", "lds+wide", "long+wide"]
    assert traces[6]["n"] + traces[6]["m"] == 510
    for t in traces[6:13]:
        assert t["runs"] >= (t["n"] + t["m"]) // 2
    for t, (d, ops) in zip(traces[10:13], want[10:13]):
        assert t["route"] == "probe" and t["n"] + t["m"] == 510 and d == 170 and t["runs"] == 340 + (t["sfx"] > 0) and "X" not in ops
    assert all(t["route"].endswith("wide") for t in traces[13:])


def _bytes_and_offsets():
    odd = bytes([0, 0x7F, 0x80, 0xFF, 0x41, 0x61])
    r = random.Random(1400)
    pairs = []
    for i in range(24):
        a = bytes(r.choice(odd) for _ in range(r.randint(1, 90)))
        b = bytearray(a)
        for _ in range(r.randint(1, 6)):
            at = r.randrange(len(b) + 1)
            if r.random() < 0.5:
                b[at:at] = bytes([r.choice(odd)])
            elif at < len(b):
                b[at] = r.choice(odd)
        pairs.append((a, bytes(b)))
        if i % 5 == 2:
            pairs.append((b"", b""))
    pairs += [(b"acgtACGT", b"ACGTacgt"), (b"\x00" * 40, b"\x80" * 37), (b"\xff" * 200 + b"\x00", b"\xff" * 130 + b"\x7f"), (b"", b"")]
    return pairs


A_OFF0, B_OFF0 = 7, 13            # where the first pair starts in the buffers the raw call is given


def _bytes_and_offsets_condition(pairs, want, traces):
    used = set(b"".join(a + b for a, b in pairs))
    assert {0, 0x7F, 0x80, 0xFF, 0x61, 0x41} <= used and A_OFF0 != B_OFF0 and A_OFF0 and B_OFF0
    empty = [i for i, (a, b) in enumerate(pairs) if not a and not b]
    assert len(empty) >= 4 and all(0 < i for i in empty) and any(pairs[i + 1][0] for i in empty[:-1])
    assert want[-4][0] == 8 and {"trivial", "lds"} <= {t["route"] for t in traces}


def _mixed_batch():
    pairs = []
    for name in CASES[:-1]:
        pairs += case(name)
    r = random.Random(1500)
    for i in range(3000):
        a = bytes(r.choice(b"ACGT") for _ in range(r.randint(0, 14)))
        kind = r.random()
        if kind < 0.4:
            b = a
        elif kind < 0.6:
            b = bytes(r.choice(b"ACGT") for _ in range(r.randint(1, 3))) + a
        else:
            b = bytearray(a)
            for _ in range(r.randint(1, 2)):                       # a base inserted, or one replaced
                at = r.randrange(len(b) + 1)
                b[at:at + r.randint(0, 1)] = bytes([r.choice(b"ACGT")])
            b = bytes(b)
        pairs.append((a, b))
    return pairs


def _mixed_batch_condition(pairs, want, traces):
    routes = {}
    for t in traces:
        routes[t["route"]] = routes.get(t["route"], 0) + 1
    assert set(routes) == {"trivial", "lds", "long", "lds+wide", "long+wide", "probe", "probe+second"}, routes
    assert routes["trivial"] >= 1000 and routes["lds"] >= 1000
    orders = [shuffled(len(pairs), sh) for sh in MIXED_SHUFFLES]
    assert orders[0] != orders[1]
    for order in orders:                                           # the few among the many, in every quarter of the batch
        where = [i * 4 // len(order) for i, p in enumerate(order) if traces[p]["route"] not in ("trivial", "lds")]
        assert set(where) == {0, 1, 2, 3} and len(where) < len(order) // 10


MIXED_SHUFFLES = (1, 2)


def shuffled(n, seed):
    order = list(range(n))
    random.Random(1600 + seed).shuffle(order)
    return order


_BUILD = dict(fast_band_edges=_fast_band_edges, delta_edges=_delta_edges, k0_clamps=_k0_clamps, lds_edge=_lds_edge, suffix=_suffix,
              wide_shapes=_wide_shapes, wide_values_edge=_wide_values_edge, probe_edges=_probe_edges, run_area=_run_area,
              bytes_and_offsets=_bytes_and_offsets, mixed_batch=_mixed_batch)
CASES = list(_BUILD)


@functools.lru_cache(maxsize=None)
def _align(a, b):
    return ec.align(a, b)


@functools.lru_cache(maxsize=None)
def _model(a, b, full):
    d, ops, tr = bm.model(a, b, known=None if full else _align(a, b))
    return d, ops, tr


@functools.lru_cache(maxsize=None)
def case(name):
    """the pairs of the case, [(a, b)] as bytes"""
    return tuple(_BUILD[name]())


def expected(name):
    """[(distance, ops)] of tests/edit_checker.py"""
    return [_align(a, b) for a, b in case(name)]


def traces(name, full=False):
    """the model's trace of every pair; full: with the deciding sweep and the traceback over the stored codes (the CPU test), else
    resting on the checker's result for them (what the GPU tests need for the counters)"""
    return [_model(a, b, full)[2] for a, b in case(name)]


def modelled(name):
    """[(distance, ops)] of the full model"""
    return [_model(a, b, True)[:2] for a, b in case(name)]


def condition(name, full=False):
    globals()[f"_{name}_condition"](case(name), expected(name), traces(name, full))


def check(name, P=bm.DEFAULT):
    """the model with parameters P (a narrowed or changed one: README_edits.md) on the case: results against the checker, then the condition"""
    pairs, want = case(name), expected(name)
    got = [_model(a, b, True) if P is bm.DEFAULT else bm.model(a, b, P) for a, b in pairs]
    bad = [i for i, g in enumerate(got) if g[:2] != want[i]]
    assert not bad, f"{name}: the model differs from the checker on pairs {bad[:10]}, e.g. distance {got[bad[0]][0]} for {want[bad[0]][0]}"
    globals()[f"_{name}_condition"](pairs, want, [g[2] for g in got])
