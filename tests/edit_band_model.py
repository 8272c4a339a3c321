"""A numpy restatement of the arithmetic of edit_kernel.hip / edit_kernel.hpp and of the host loop around it (hypo_gpu_edit_scripts in
capi.hip), written from those files and not from tests/edit_checker.py: the suffix trim by ballots of 64, the shortcuts, edit_fast_k0,
the banded anti-diagonal sweep with the kernels' tie order (diagonal, up, left) and EDIT_INF outside the band, the exactness test,
edit_wide_band / edit_wide_groups, the probe and the second pass, and the traceback that reads its move codes from the very words
it writes its runs into.  model(a, b) gives (distance, ops, trace); the trace says which way the pair went, so that a case can
assert that it reaches what it is there for, and batch_counts() predicts hypo_gpu_edit_last_counts from the traces alone.

The constants are stated here, not imported; tests/test_edit_band_model_cpu.py compares them with edit_kernel.hpp.  Params also
narrows them (band 8, ...) so that every route is met on inputs small enough to enumerate, and carries the one-line changes of
tests/README_edits.md (`mut`), each of which some test must notice."""
from collections import namedtuple

import numpy as np

INF = 1 << 29
OPS = "=XDI"

_Params = namedtuple("Params", "band lds_steps lds_diags probe_h threads mut")


def Params(band=128, lds_steps=512, lds_diags=8192, probe_h=64, threads=256, mut=()):
    """band: EDIT_FAST_BAND (a wave is band / 2 lanes); lds_steps: EDIT_LDS_STEPS; lds_diags: EDIT_WIDE_LDS_DIAGS; probe_h:
    EDIT_PROBE_H; threads: EDIT_WIDE_THREADS"""
    assert band % 2 == 0 and threads % (band // 2) == 0
    return _Params(band, lds_steps, lds_diags, probe_h, threads, frozenset([mut] if isinstance(mut, str) else mut))


DEFAULT = Params()
NARROW = Params(band=8, lds_steps=16, lds_diags=12, probe_h=2, threads=4)
CHUNK_BYTES = 256 << 20


def fresh_pool_runs(n_pairs):
    """the run pool a fresh context gives a call: 4 runs per pair + 1024, and the quarter of head room every device buffer gets"""
    return 5 * n_pairs + 1280


MUTATIONS = ("exact_lo_loose", "exact_lo_strict", "exact_hi_loose", "exact_hi_strict", "h_round_up", "h_minus_1", "lane0_inf", "lane63_inf",
             "tie_swap", "tie_swap_wide", "delta_ge", "delta_gt_band", "suffix_edge", "k0_clamp_lo", "k0_clamp_hi", "probe_h_once", "second_d_minus_1",
             "s_half", "g_floor", "g_guard")


def suffix(a, b, P=DEFAULT):
    """edit_suffix: the common suffix, found in chunks of one wave's ballot"""
    n, m = len(a), len(b)
    mn, L = min(n, m), P.band // 2
    for c in range(0, mn, L):
        q = np.arange(c, c + L)
        ok = q < mn
        qa = np.where(ok, n - 1 - q, 0)
        qb = np.where(ok, m - 1 - q, 0)
        diff = np.where(ok, a[qa] != b[qb], True)
        if diff.any():
            s = c + int(np.argmax(diff))
            if "suffix_edge" in P.mut and s == c and 0 < s < mn:
                s += 1
            return s
    return mn


def fast_k0(n, m, P=DEFAULT):
    delta = m - n
    ad = abs(delta)
    K0 = min(0, delta) - (P.band - 1 - ad) // 2        # (C++ truncation = floor here: ad <= band - 1)
    assert ad <= P.band - 1 or "delta_gt_band" in P.mut
    if K0 < -n:
        if "k0_clamp_lo" not in P.mut:
            K0 = -n
    elif K0 + P.band - 1 > m:
        if "k0_clamp_hi" not in P.mut:
            K0 = max(-n, m - P.band + 1)
    return K0


def wide_band(n, m, d, P=DEFAULT):
    delta = m - n
    ad = abs(delta)
    h = (d - ad) // 2
    assert d >= ad
    if "h_round_up" in P.mut:
        h = (d - ad + 1) // 2
    if "h_minus_1" in P.mut:
        h -= 1
    return max(-n, min(0, delta) - h), min(m, max(0, delta) + h)


def wide_groups(lo, hi, P=DEFAULT):
    L = P.band // 2
    if "g_floor" in P.mut:
        return ((hi - lo + 2) // 2) // L
    return ((hi - lo + 2) // 2 + L - 1) // L


def required_band(n, m, d, P=DEFAULT):
    """[lo_req, hi_req] of the exactness test: where every path of cost <= d lies"""
    return wide_band(n, m, d, P)


class Storage:
    """the move storage of one pair: words of 64 bits to the sweep and the code reader, words of 32 bits to the run writer.  An
    index outside it is an error here (on the device it is another pair's storage, or LDS of another wave)."""

    def __init__(self, n_bytes):
        assert n_bytes % 16 == 0
        self.buf = np.zeros(n_bytes, dtype=np.uint8)
        self.w64 = self.buf.view(np.uint64)
        self.w32 = self.buf.view(np.uint32)

    def check(self, view, i):
        if not 0 <= i < view.size:
            raise IndexError(f"move storage: word {i} of {view.size}")
        return i


def sweep(A, B, n, m, lo, hi, G, st, P, wide):
    """Anti-diagonals t = 0 .. n + m over the diagonals [lo, hi]; slot s owns the diagonals lo + 2s and lo + 2s + 1, and step t computes
    the one with the parity of t.  The 2-bit codes of step t are stored as G groups of two ballots at 64-bit words 2 (t G + g).
    Returns the band's values after the last step, indexed by diagonal - lo."""
    W = hi - lo + 1
    L = P.band // 2
    S = W // 2 if "s_half" in P.mut else (W + 1) // 2
    slots = (-(-S // P.threads) * P.threads) if wide else L           # slots that ballot: C x threads, or one wave
    n_groups = slots // L
    V = np.full(W + 2, INF, dtype=np.int64)                            # V[1 + k - lo]; V[0] and V[W + 1] stay INF: outside the band
    T = n + m
    sl = np.arange(slots)
    bits = np.zeros((2, n_groups * L), dtype=np.uint8)
    for t in range(T + 1):
        par = (t + lo) & 1
        k = lo + 2 * sl + par
        live = (sl < S) & (k <= hi)
        ti, tj = t - k, t + k
        i, j = ti >> 1, tj >> 1
        cell = live & (ti >= 0) & (tj >= 0) & (i <= n) & (j <= m)
        inner = cell & (i > 0) & (j > 0)
        ix = np.nonzero(inner)[0]
        v = np.full(slots, INF, dtype=np.int64)
        c = np.zeros(slots, dtype=np.uint8)
        top_row = cell & (i == 0)
        left_col = cell & (i > 0) & (j == 0)
        v[top_row] = j[top_row]; c[top_row] = 3
        v[left_col] = i[left_col]; c[left_col] = 2
        if ix.size:
            kk = k[ix] - lo + 1
            x = (A[i[ix] - 1] != B[j[ix] - 1]).astype(np.int64)
            dg = V[kk] + x
            up = V[kk + 1]
            left = V[kk - 1]
            if not wide:
                # the fast kernel's neighbour comes from __shfl_down / __shfl_up, which hand a wave's last / first lane its own value
                if "lane63_inf" in P.mut:
                    up = np.where(kk == W, V[kk - 1], up)
                if "lane0_inf" in P.mut:
                    left = np.where(kk == 1, V[kk + 1], left)
            u, le = up + 1, left + 1
            vv = np.minimum(dg, np.minimum(u, le))
            if ("tie_swap_wide" if wide else "tie_swap") in P.mut:
                cc = np.where(vv == dg, x, np.where(vv == le, 3, 2))
            else:
                cc = np.where(vv == dg, x, np.where(vv == u, 2, 3))
            v[ix] = vv
            c[ix] = cc
        lv = np.nonzero(live)[0]
        V[k[lv] - lo + 1] = v[lv]
        bits[0] = c & 1
        bits[1] = c >> 1
        words = np.packbits(bits.reshape(2, n_groups, L), axis=2, bitorder="little")      # [2, groups, L / 8] bytes
        w = np.zeros((n_groups, 2, 8), dtype=np.uint8)
        w[:, :, :(L + 7) // 8] = words.transpose(1, 0, 2)
        w = w.reshape(n_groups, 16).view(np.uint64)                                          # [groups, 2]
        keep = n_groups if "g_guard" in P.mut else min(G, n_groups)                          # the kernel's `g < G`
        st.check(st.w64, 2 * t * G)
        st.check(st.w64, 2 * (t * G + keep) - 1)
        st.w64[2 * t * G:2 * (t * G + keep)] = w[:keep].reshape(-1)
    return V[1:W + 1]


def traceback(st, n, m, sfx, lo, G, P):
    """edit_traceback over the stored codes: the runs go backwards from 32-bit word `top` of the same storage.  (ops, number of runs)"""
    L = P.band // 2
    top = 4 * G * (n + m + 2) - 1
    R = 0

    def put(word):
        nonlocal R
        st.w32[st.check(st.w32, top - R)] = word
        R += 1

    def code(i, j):
        t = i + j
        par = (t + lo) & 1
        s = (j - i - lo - par) >> 1
        if s < 0 or s // L >= G:
            raise IndexError(f"move code of diagonal {j - i}: slot {s}, {G} groups")
        at = 2 * (t * G + s // L)
        b = s % L
        return ((int(st.w64[st.check(st.w64, at)]) >> b) & 1) | (((int(st.w64[st.check(st.w64, at + 1)]) >> b) & 1) << 1)

    if sfx:
        put((sfx << 2) | 0)
    i, j, cur, ln = n, m, 4, 0
    while i | j:
        op = 3 if i == 0 else 2 if j == 0 else code(i, j)
        if op != cur:
            if ln:
                put((ln << 2) | cur)
            cur, ln = op, 0
        ln += 1
        if op < 2:
            i -= 1; j -= 1
        elif op == 2:
            i -= 1
        else:
            j -= 1
    if ln:
        put((ln << 2) | cur)
    runs = [int(x) for x in st.w32[top + 1 - R:top + 1]]
    return "".join(OPS[r & 3] * (r >> 2) for r in runs), R


def exactness(n, m, d, lo, hi, P, fast):
    lo_req, hi_req = required_band(n, m, d, P)
    lo_ok, hi_ok = lo_req >= lo, hi_req <= hi
    if fast:
        if "exact_lo_loose" in P.mut: lo_ok = lo_req >= lo - 1
        if "exact_lo_strict" in P.mut: lo_ok = lo_req > lo
        if "exact_hi_loose" in P.mut: hi_ok = hi_req <= hi + 1
        if "exact_hi_strict" in P.mut: hi_ok = hi_req < hi
    return lo_ok and hi_ok, lo_req, hi_req


def model(a, b, P=DEFAULT, known=None):
    """(distance, ops, trace) of one pair as the device computes it.  known = (distance, ops) from elsewhere: the sweep that decides
    the pair (the most expensive one of a wide pair) is left out and the trace, which then rests on `known`, is the same: what a
    GPU test needs for batch_counts() of pairs whose full model the CPU test has already held against the checker.  trace: sfx, n, m (trimmed), route, runs, passes: one dict per
    sweep with kind ('fast' | 'wide' | 'probe' | 'second'), lo, hi, W, d_b, exact, lo_req, hi_req, and for the fast pass K0 and lds,
    for a wide pass bound, S, G, C, dropped (ballots per step the g < G guard drops), vals_lds; moves_bytes / vals_bytes: what the
    host asks for (0: LDS)."""
    A0 = np.frombuffer(bytes(a), dtype=np.uint8)
    B0 = np.frombuffer(bytes(b), dtype=np.uint8)
    sfx = suffix(A0, B0, P)
    n, m = A0.size - sfx, B0.size - sfx
    A, B = A0[:n], B0[:m]
    tr = dict(sfx=sfx, n=n, m=m, passes=[])
    if n == 0 or m == 0:
        tr.update(route="trivial", runs=(n > 0) + (m > 0) + (sfx > 0))
        return n + m, "D" * n + "I" * m + "=" * sfx, tr
    delta, L = m - n, P.band // 2
    ad = abs(delta)
    to_probe = ad >= P.band - 1 if "delta_ge" in P.mut else ad > P.band if "delta_gt_band" in P.mut else ad > P.band - 1
    if to_probe:
        route, bound, kind = "probe", ad + (1 if "probe_h_once" in P.mut else 2) * P.probe_h, "probe"
    else:
        lds = n + m + 2 <= P.lds_steps
        route = "lds" if lds else "long"
        K0 = fast_k0(n, m, P)
        nbytes = 16 * (n + m + 2)
        st = Storage(16 * P.lds_steps if lds else nbytes)
        V = sweep(A, B, n, m, K0, K0 + P.band - 1, 1, st, P, wide=False)
        if not 0 <= delta - K0 < P.band:
            raise IndexError(f"diagonal {delta} outside the band at {K0}")
        d = int(V[delta - K0])
        exact, lo_req, hi_req = exactness(n, m, d, K0, K0 + P.band - 1, P, fast=True)
        tr["passes"].append(dict(kind="fast", K0=K0, lo=K0, hi=K0 + P.band - 1, W=P.band, d_b=d, exact=exact, lo_req=lo_req, hi_req=hi_req,
                                 lds=lds, moves_bytes=0 if lds else nbytes, vals_bytes=0))
        if exact:
            ops, R = traceback(st, n, m, sfx, K0, 1, P)
            tr.update(route=route, runs=R)
            return d, ops, tr
        route, bound, kind = route + "+wide", d, "wide"
    while True:
        lo, hi = wide_band(n, m, bound, P)
        W = hi - lo + 1
        S = W // 2 if "s_half" in P.mut else (W + 1) // 2
        G, C = wide_groups(lo, hi, P), -(-S // P.threads)
        if known is not None and kind != "probe":
            d = known[0]
        else:
            st = Storage(16 * G * (n + m + 2))
            V = sweep(A, B, n, m, lo, hi, G, st, P, wide=True)
            d = int(V[delta - lo])
        exact, lo_req, hi_req = exactness(n, m, d, lo, hi, P, fast=False) if kind == "probe" else (True, lo, hi)
        tr["passes"].append(dict(kind=kind, bound=bound, lo=lo, hi=hi, W=W, S=S, G=G, C=C, dropped=C * (P.threads // L) - G, d_b=d, exact=exact,
                                 lo_req=lo_req, hi_req=hi_req, vals_lds=W <= P.lds_diags, moves_bytes=16 * G * (n + m + 2),
                                 vals_bytes=0 if W <= P.lds_diags else 4 * W))
        if exact:
            break
        route, bound, kind = "probe+second", d - (1 if "second_d_minus_1" in P.mut else 0), "second"
    if known is not None:
        ops = known[1]
        R = sum(1 for i, o in enumerate(ops) if i == 0 or ops[i - 1] != o)
    else:
        ops, R = traceback(st, n, m, sfx, lo, G, P)
    tr.update(route=route, runs=R)
    return d, ops, tr


def chunks(needs, chunk_bytes):
    """edit_run_list: launches of a list whose entries need `needs` bytes of move storage, in list order"""
    launches, e0 = 0, 0
    while e0 < len(needs):
        mb, e1 = 0, e0
        while e1 < len(needs) and not (e1 > e0 and mb + needs[e1] > chunk_bytes):
            mb += (needs[e1] + 15) & ~15
            e1 += 1
        launches, e0 = launches + 1, e1
    return launches


def batch_counts(traces, chunk_bytes=CHUNK_BYTES, pool_runs=None):
    """hypo_gpu_edit_last_counts of a call whose pairs have these traces.  The device fills its lists in any order and the host
    chunks them first-fit in that order, so `long_launches` / `wide_launches` are one number where the order cannot matter (the list
    fits one chunk; every entry needs the same; or all but one do, and every place of the odd one gives the same count) and a
    (min, max) pair otherwise.  pool_runs: the run pool the context has (None: a fresh context's,
    fresh_pool_runs); passes is 2 when the runs do not fit it."""
    n = len(traces)
    by = lambda kind: [p["moves_bytes"] for t in traces for p in t["passes"] if p["kind"] == kind]
    long_needs = [p["moves_bytes"] for t in traces for p in t["passes"] if p["kind"] == "fast" and not p["lds"]]
    first = by("wide") + by("probe")
    second = by("second")
    runs = sum(t["runs"] for t in traces)
    pool = fresh_pool_runs(n) if pool_runs is None else pool_runs

    def launches(needs):
        if not needs:
            return 0
        if len(set(needs)) == 1 or sum(needs) <= chunk_bytes:
            return chunks(needs, chunk_bytes)
        kinds = sorted(set(needs), key=needs.count)
        if len(kinds) == 2 and needs.count(kinds[0]) == 1:
            rest = [kinds[1]] * (len(needs) - 1)
            got = {chunks(rest[:at] + [kinds[0]] + rest[at:], chunk_bytes) for at in range(len(needs))}
            return min(got) if len(got) == 1 else (min(got), max(got))
        return (1, len(needs))

    def add(x, y):
        if isinstance(x, tuple) or isinstance(y, tuple):
            x, y = (x if isinstance(x, tuple) else (x, x)), (y if isinstance(y, tuple) else (y, y))
            return (x[0] + y[0], x[1] + y[1])
        return x + y
    return dict(pairs=n, long=len(long_needs), wide=len(first), second=len(second), runs=runs, passes=2 if runs > pool else 1,
                long_launches=launches(long_needs), wide_launches=add(launches(first), launches(second)))


def counts_match(got, want):
    """got: edit_last_counts(); want: batch_counts(); a (min, max) of want admits any value between"""
    return all(want[k][0] <= got[k] <= want[k][1] if isinstance(want[k], tuple) else got[k] == want[k] for k in want)
