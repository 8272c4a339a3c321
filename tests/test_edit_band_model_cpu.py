"""CPU: tests/edit_band_model.py (the arithmetic of edit_kernel.hip restated in numpy, with the route each pair takes) against
tests/edit_checker.py on every case of tests/edit_cases.py — the inputs tests/test_gpu_edit_direct.py hands the kernels — and every
case's condition; the model's constants against edit_kernel.hpp and its band functions against the C++ ones; the model with
narrowed constants on every pair over {A, C} up to length 6; and the one-line changes of tests/README_edits.md, each of which must
fail a named case or be shown to change nothing."""
import ctypes as C
import itertools
import os
import re

import pytest

import edit_band_model as bm
import edit_cases as cases
from hypo_amd import capi
from test_edit_checker_cpu import canonical_brute

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", cases.CASES)
def test_the_model_equals_the_checker_and_the_case_reaches_its_edge(name):
    """distance and ops of every pair, with the deciding sweep and the traceback over the stored codes; then the condition"""
    cases.check(name)
    # what the GPU tests use for the counters — the trace without the deciding sweep, resting on the checker's result — is the same trace
    assert cases.traces(name, full=False) == cases.traces(name, full=True)


def test_every_wide_pass_has_more_than_one_group():
    """a pair the fast band could not decide needs more than 128 diagonals, so G >= 2 and the ballots a step writes beyond G
    (`g < G` dropped, README_edits.md) would stay inside the next step's words or the spare anti-diagonal"""
    for name in cases.CASES[:-1]:
        for t in cases.traces(name, full=True):
            for p in [p for p in t["passes"] if p["kind"] != "fast"]:
                assert p["W"] >= 129 and p["G"] >= 2 and p["C"] * 4 <= 2 * p["G"], (name, p)


def test_constants_match_the_header():
    src = open(os.path.join(ROOT, "hypo_amd", "csrc", "edit_kernel.hpp")).read()
    val = lambda n: int(re.search(r"constexpr\s+uint32_t\s+%s\s*=\s*(\d+)\s*;" % n, src).group(1))
    P = bm.DEFAULT
    assert (P.band, P.lds_steps, P.lds_diags, P.probe_h, P.threads) == (128, 512, 8192, 64, 256)
    assert (val("EDIT_FAST_BAND"), val("EDIT_LDS_STEPS"), val("EDIT_WIDE_LDS_DIAGS"), val("EDIT_PROBE_H"), val("EDIT_WIDE_THREADS")) == (128, 512, 8192, 64, 256)
    kernel = open(os.path.join(ROOT, "hypo_amd", "csrc", "edit_kernel.hip")).read()
    assert re.search(r"constexpr\s+int\s+EDIT_INF\s*=\s*1\s*<<\s*29\s*;", kernel) and bm.INF == 1 << 29
    host = open(os.path.join(ROOT, "hypo_amd", "csrc", "capi.hip")).read()
    assert re.search(r"g_edit_chunk_bytes\{\(uint64_t\)256 << 20\}", host) and bm.CHUNK_BYTES == 256 << 20


def test_band_functions_match_the_cxx_ones():
    """edit_wide_band / edit_wide_groups as g++ compiles them (hypo_host_edit_wide_band / _groups in host_capi.cpp).  edit_fast_k0 is
    device code of edit_kernel.hip and cannot be called from the host: test_gpu_edit_direct.py holds it through the routes
    (k0_clamps) and the counters."""
    from hypo_amd import host
    if not os.path.exists(host.LIB_PATH):
        capi.build_library()
    lib = C.CDLL(host.LIB_PATH)
    lib.hypo_host_edit_wide_groups.restype = C.c_uint64
    lo, hi = C.c_int64(), C.c_int64()
    sizes = [0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 130, 255, 256, 300, 511, 512, 8191, 8192, 20000]
    n_checked = 0
    for n, m in itertools.product(sizes, sizes):
        ad = abs(m - n)
        for d in sorted({ad, ad + 1, ad + 2, ad + 3, ad + 126, ad + 127, ad + 128, ad + 129, ad + 130, max(n, m), n + m}):
            if d < ad or d > n + m:
                continue
            lib.hypo_host_edit_wide_band(C.c_uint32(n), C.c_uint32(m), C.c_uint32(d), C.byref(lo), C.byref(hi))
            assert (lo.value, hi.value) == bm.wide_band(n, m, d), (n, m, d)
            assert lib.hypo_host_edit_wide_groups(lo, hi) == bm.wide_groups(lo.value, hi.value), (n, m, d)
            n_checked += 1
    assert n_checked > 2000


SMALL = [bytes(x) for n in range(7) for x in itertools.product(b"AC", repeat=n)]


def sweep_small(P):
    routes = {}
    for a in SMALL:
        for b in SMALL:
            d, ops, tr = bm.model(a, b, P)
            assert (d, ops) == canonical_brute(a.decode(), b.decode()), (a, b, tr)
            routes[tr["route"]] = routes.get(tr["route"], 0) + 1
    return routes


def test_every_pair_up_to_length_6_with_a_band_of_8():
    """band 8, 16 LDS steps, probe h 2, 4 wide threads.  With these numbers every pair of at most 6 + 6 bytes still fits the band and
    the LDS steps (|m - n| <= 6 < 8; h <= 3; n + m + 2 <= 14), so only `trivial` and `lds` are met; the next test narrows further."""
    assert set(sweep_small(bm.NARROW)) == {"trivial", "lds"}


def test_every_pair_up_to_length_6_with_a_band_of_4():
    """band 4, 10 LDS steps, band values in LDS up to 6 diagonals, probe h 0, 2 wide threads: the same code meets every route"""
    routes = sweep_small(bm.Params(band=4, lds_steps=10, lds_diags=6, probe_h=0, threads=2))
    assert set(routes) == {"trivial", "lds", "long", "lds+wide", "long+wide", "probe", "probe+second"}, routes


# ---- the one-line changes of README_edits.md ----------------------------------------------------------------------------------------

CAUGHT_BY = dict(exact_lo_loose="fast_band_edges", exact_lo_strict="fast_band_edges", exact_hi_strict="fast_band_edges", h_round_up="fast_band_edges",
                 h_minus_1="fast_band_edges", lane63_inf="k0_clamps", tie_swap="k0_clamps", tie_swap_wide="wide_shapes", delta_ge="delta_edges",
                 delta_gt_band="delta_edges", suffix_edge="suffix", k0_clamp_lo="k0_clamps", probe_h_once="delta_edges", second_d_minus_1="probe_edges",
                 s_half="fast_band_edges", g_floor="fast_band_edges")
EQUIVALENT = ("exact_hi_loose", "k0_clamp_hi", "lane0_inf", "g_guard")


def test_every_change_is_listed():
    assert sorted(list(CAUGHT_BY) + list(EQUIVALENT)) == sorted(bm.MUTATIONS)
    readme = open(os.path.join(ROOT, "tests", "README_edits.md")).read()
    for mut in bm.MUTATIONS:
        assert f"`{mut}`" in readme, mut


@pytest.mark.parametrize("mut", sorted(CAUGHT_BY))
def test_a_changed_model_fails_its_case(mut):
    """the case named fails — a result that differs from the checker, an index outside the storage, or the condition — and passes unchanged"""
    cases.check(CAUGHT_BY[mut])
    with pytest.raises((AssertionError, IndexError)):
        cases.check(CAUGHT_BY[mut], bm.Params(mut=mut))


def test_the_second_bound_of_the_exactness_test_never_decides():
    """`hi_req <= K0 + 127` as `<= K0 + 128` (exact_hi_loose) changes no outcome: the centred band has at least as much room above
    max(0, D) as below min(0, D), and where K0 is clamped to -n the band reaches m.  Every n, m up to 200, and the distances around
    the one at which the first bound turns (and the smallest and the largest)."""
    loose = bm.Params(mut="exact_hi_loose")
    for n in range(1, 201):
        for m in range(max(1, n - 127), min(200, n + 127) + 1):
            K0, ad = bm.fast_k0(n, m), abs(m - n)
            turn = ad + 2 * ((127 - ad) // 2)
            for d in sorted({ad, n + m} | {x for x in range(turn - 2, turn + 6) if ad <= x <= n + m}):
                assert bm.exactness(n, m, d, K0, K0 + 127, bm.DEFAULT, True)[0] == bm.exactness(n, m, d, K0, K0 + 127, loose, True)[0], (n, m, d)


def test_the_second_clamp_of_k0_never_moves_it():
    """edit_fast_k0's `else if (K0 + 127 > m)` is entered only with n + m = 126, and max(-n, m - 127) is then the K0 it had
    (k0_clamp_hi): every n, m whose |m - n| the band holds, up to 400"""
    dropped = bm.Params(mut="k0_clamp_hi")
    entered = set()
    for n in range(1, 401):
        for m in range(max(1, n - 127), min(400, n + 127) + 1):
            assert bm.fast_k0(n, m) == bm.fast_k0(n, m, dropped), (n, m)
            free = min(0, m - n) - (127 - abs(m - n)) // 2
            if free >= -n and free + 127 > m:
                entered.add(n + m)
    assert entered == {126}


@pytest.mark.parametrize("mut", ["lane0_inf", "g_guard"])
def test_two_changes_that_cannot_show(mut):
    """lane0_inf: without `lane == 0 ? EDIT_INF`, __shfl_up hands lane 0 its own value, which is the `up` term of the same cell: left + 1
    equals up + 1, the minimum is the same and `up` wins the tie as before.  g_guard: see test_every_wide_pass_has_more_than_one_group.
    The model, changed the way the hardware would behave, gives the same results on the cases that reach the place."""
    for name in ("k0_clamps", "fast_band_edges", "delta_edges", "run_area"):
        cases.check(name, bm.Params(mut=mut))
