// sched_cases.cpp — TEST-ONLY C interface to hypo_amd/csrc/poa_sched.hpp (the host's scheduling decisions of poa_run), so that
// tests/test_poa_schedule_cpu.py can pin them without a GPU.  Built by tests/emu/Makefile into tests/_build/libhypo_sched[_asan].so.
// The knobs are read from the caller's environment (PoaKnobs::from_env), as poa_run reads them.  Not part of the product.
#include "../../hypo_amd/csrc/poa_sched.hpp"

using namespace hypo;

extern "C" {

// sizes of the structures the test mirrors with ctypes
void sched_sizes(uint64_t out[4]) { out[0] = sizeof(PoaHistory); out[1] = sizeof(PoaSchedule); out[2] = sizeof(PoaPinned); out[3] = sizeof(PoaWorkspaceLayout); }

void sched_layout(uint32_t n_windows, PoaWorkspaceLayout* out) { *out = poa_workspace_layout(n_windows); }

void sched_history(const PoaPinned* pinned, int have_history, int waited, const uint32_t prev_planned[8], uint32_t n_windows,
                   uint32_t history_windows, PoaHistory* out) {
    *out = poa_history(pinned, have_history != 0, waited != 0, prev_planned, n_windows, history_windows);
}

// fp: five footprints {lds, vgprs, max_waves} (class 0 with four groups, with two, classes 1, 2, 3); lanes per group 16 / 32 as in the product
void sched_schedule(const PoaHistory* h, uint32_t n_windows, int groups4, const int64_t fp[15], PoaSchedule* out) {
    auto f = [&](int i) { return WaveFootprint{(size_t)fp[3 * i], (int)fp[3 * i + 1], (int)fp[3 * i + 2]}; };
    const PoaFootprints F = {f(0), f(1), f(2), f(3), f(4), 16, 32};
    *out = poa_schedule(*h, n_windows, groups4, PoaKnobs::from_env(), F);
}

uint32_t sched_late_arrivals(const PoaHistory* h, int cls, uint32_t n_windows) { return late_arrivals(*h, cls, n_windows); }
uint32_t sched_rare_grid_hint(const PoaHistory* h, int cls, uint32_t n_windows) { return rare_grid_hint(*h, cls, n_windows); }
int sched_side_by_side(int groups3, uint32_t poll_groups) { return poa_side_by_side(groups3, poll_groups) ? 1 : 0; }

long sched_grid(int occupancy, int cap, int num_cus, int groups_per_wave, int clamp_groups, int group_cap, uint32_t n_windows) {
    return poa_grid(occupancy, PoaKnobs::from_env().waves_per_cu, cap, num_cus, groups_per_wave, clamp_groups != 0, group_cap, n_windows);
}

}  // extern "C"
