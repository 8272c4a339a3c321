// sched_main_cases.cpp — TEST-ONLY C interface to the part of hypo_amd/csrc/poa_sched.hpp that decides which first pass rides the
// caller's stream (PoaSchedule::main_class), for tests/test_poa_schedule_main_cpu.py, which builds it with g++ into
// tests/_build/libhypo_sched_main.so.  The knobs are read from the caller's environment, as poa_run reads them.  Not part of the product.
#include "../../hypo_amd/csrc/poa_sched.hpp"

using namespace hypo;

extern "C" {

// sizeof(PoaSchedule) and the offsets of the fields around the new byte
void sched_main_layout(uint64_t out[5]) {
    out[0] = sizeof(PoaSchedule); out[1] = offsetof(PoaSchedule, long_first_pass); out[2] = offsetof(PoaSchedule, main_class);
    out[3] = offsetof(PoaSchedule, first4); out[4] = offsetof(PoaSchedule, mopup4);
}

// planned[3], work[3], lanes per group of class 0 in the measured call, valid -> main_class (and the rest of the schedule through *out);
// footprints as in tests/test_poa_schedule_cpu.py, lanes per group 16 / 32 as in the product
int sched_main(const uint32_t planned[3], const uint64_t work[3], uint64_t measured_gw, int valid, uint32_t n_windows, PoaSchedule* out) {
    PoaHistory h = {};
    for (int c = 0; c < 3; ++c) { h.planned[c] = h.last_count[c] = h.last_planned[c] = planned[c]; h.work[c] = work[c]; }
    h.measured_gw = measured_gw;
    h.valid = valid != 0;
    const PoaFootprints F = {{15872, 96, 10}, {8192, 96, 10}, {8192, 128, 8}, {14848, 128, 8}, {16384, 128, 8}, 16, 32};
    *out = poa_schedule(h, n_windows, 2048, PoaKnobs::from_env(), F);
    return out->main_class;
}

}  // extern "C"
