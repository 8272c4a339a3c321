// poa_sched.hpp — the host's decisions about a POA call, as plain data: workspace layout, tuning knobs, what the last call left
// behind, and the schedule poa_run (poa_kernel.hip) then only has to enqueue.  No HIP here: tests/emu/sched_cases.cpp compiles
// this header with g++ and tests/test_poa_schedule_cpu.py pins its answers without a GPU.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

namespace hypo {

constexpr int kPoaSchedClasses = 6;                   // = kNumPoaClasses (poa_kernel.hip asserts it)
constexpr size_t kPoaHeaderBytes = 8192;              // head of the workspace: the kPoaHdr* fields of poa_kernel.hpp
// resident groups of class 3 (direction codes in HBM scratch, PoaLayout::DIRG_BYTES each): what 256 CUs hold at 10 waves per CU
constexpr int kMaxGroups3 = 2560;
constexpr size_t kGroup3DirgBytes = 33280;            // = PoaLayout<PoaClass3>::DIRG_BYTES (poa_kernel.hip asserts it)
constexpr uint32_t kSequentialDivisor = 10;           // class kernels one after the other when the last call left more than 1/10 of its windows to class 3

// ------------------------------------------------------------------------------------------------
// workspace: header | class queues | plan keys | carry words | spill pool | class 3's direction codes | scratch of classes 4 / 5
// ------------------------------------------------------------------------------------------------
struct PoaWorkspaceLayout {
    size_t queues, keys, carry, spill, dirg3, scratch;     // byte offsets, each a multiple of 256
    size_t spill_bytes;
    int groups3;                                            // direction-code slices at dirg3
    size_t prefix;                                          // everything in front of the scratch (= scratch)
};
inline size_t poa_align256(size_t b) { return (b + 255) / 256 * 256; }
// spill pool of the re-queued windows' graphs (Poa::spill: 1.5 KB for a class-0 window, 12 KB for a full class-3 one): a bump
// allocator, a window that finds it full starts again from its first sequence as before
inline size_t poa_spill_bytes(uint32_t n_windows) {
    size_t b = (size_t)n_windows * 1024;         // (256 until round 6: a batch in which a fifth of the windows outgrow their class ran out, and what found no room started over)
    const size_t lo = (size_t)1 << 20, hi = (size_t)1 << 30;
    return b < lo ? lo : (b > hi ? hi : b);
}
inline PoaWorkspaceLayout poa_workspace_layout(uint32_t n_windows) {
    PoaWorkspaceLayout L;
    L.queues = kPoaHeaderBytes;
    L.keys = poa_align256(L.queues + (size_t)kPoaSchedClasses * n_windows * sizeof(uint32_t));
    L.carry = L.keys + poa_align256((size_t)n_windows * 2);
    L.spill = L.carry + poa_align256((size_t)n_windows * 4);
    L.spill_bytes = poa_spill_bytes(n_windows);
    L.dirg3 = L.spill + L.spill_bytes;
    L.groups3 = n_windows < (uint32_t)kMaxGroups3 ? (n_windows < 16u ? 16 : (int)n_windows) : kMaxGroups3;
    L.scratch = L.prefix = L.dirg3 + (size_t)L.groups3 * kGroup3DirgBytes;
    return L;
}

// ------------------------------------------------------------------------------------------------
// knobs: every HYPO_POA_* variable, read once at the top of each poa_run (tests flip HYPO_POA_CLASS0 between calls).  DESIGN.md 3.1
// ------------------------------------------------------------------------------------------------
struct PoaKnobs {
    int class0 = -1;             // HYPO_POA_CLASS0=16|32: lanes per group of class 0 (-1: the plan decides)
    int sequential = -1;         // HYPO_POA_SEQUENTIAL=0|1 (-1: the history decides)
    bool sync_plan = false;      // HYPO_POA_SYNC_PLAN (set at all): every call waits for its own plan
    bool caps_set = false;       // HYPO_POA_CAPS=c0,c1,c2[,c3[,c4]]: waves per CU of classes 0 - 2 (wins over both rules and over adapt), c3: of the polling launch
    int caps[kPoaSchedClasses] = {5, 5, 5, 0, 0, 0};
    char order[4] = "201";       // HYPO_POA_ORDER: submission order of the three first passes
    bool poll = true;            // HYPO_POA_POLL=0: no polling launch of class 3
    bool poll_waves_set = false; // HYPO_POA_POLL_WAVES: its size
    uint32_t poll_waves = 0;
    int adapt = -1;              // HYPO_POA_ADAPT=0|1: wave shares from the last call's work never / everywhere (-1: four-group batches)
    bool adapt_log = false;      // HYPO_POA_ADAPT_LOG: print the shares picked
    int waves_per_cu = 0;        // HYPO_POA_WAVES_PER_CU: cap on every launch (tuning / diagnostics)
    int main_class = -1;         // HYPO_POA_MAIN=0|1|2: the first pass that goes on the caller's stream (-1: the history decides)
    static PoaKnobs from_env() {
        PoaKnobs k;
        if (const char* v = getenv("HYPO_POA_CLASS0")) k.class0 = atoi(v);
        if (const char* v = getenv("HYPO_POA_SEQUENTIAL")) k.sequential = atoi(v) > 0;
        k.sync_plan = getenv("HYPO_POA_SYNC_PLAN") != nullptr;
        if (const char* v = getenv("HYPO_POA_CAPS")) { k.caps_set = true; sscanf(v, "%d,%d,%d,%d,%d", &k.caps[0], &k.caps[1], &k.caps[2], &k.caps[3], &k.caps[4]); }
        if (const char* v = getenv("HYPO_POA_ORDER")) if (strlen(v) == 3) memcpy(k.order, v, 3);
        if (const char* v = getenv("HYPO_POA_POLL")) k.poll = atoi(v) != 0;
        if (const char* v = getenv("HYPO_POA_POLL_WAVES")) { k.poll_waves_set = true; k.poll_waves = (uint32_t)atoi(v); }
        if (const char* v = getenv("HYPO_POA_ADAPT")) k.adapt = atoi(v) != 0;
        k.adapt_log = getenv("HYPO_POA_ADAPT_LOG") != nullptr;
        if (const char* v = getenv("HYPO_POA_WAVES_PER_CU")) k.waves_per_cu = atoi(v);
        if (const char* v = getenv("HYPO_POA_MAIN")) if (v[0] >= '0' && v[0] <= '2' && !v[1]) k.main_class = v[0] - '0';
        return k;
    }
};

// ------------------------------------------------------------------------------------------------
// history: what the kernels leave in page-locked host memory, and what a call reads out of it
// ------------------------------------------------------------------------------------------------
// PoaAux::pinned.  poa_plan_count_kernel (its last workgroup) writes `plan`, poa_giant_kernel (the last launch of a call) `final_count` and `work`: no
// copy commands on the stream, and whoever reads gets the last finished call.
struct PoaPinned {
    uint32_t plan[8];            // planned counts per class of the call in flight
    uint32_t final_count[8];     // final counts of the last finished call
    uint32_t unused[8];
    uint64_t work[8];            // its wave-time per class (PoaQueues::work); [6]: lanes per group of class 0 in that call
};
constexpr int kPinnedGeometrySlot = 6;
static_assert(offsetof(PoaPinned, final_count) == 8 * 4 && offsetof(PoaPinned, work) == 24 * 4 && sizeof(PoaPinned) == 40 * 4, "the kernels' view of the block");

struct PoaHistory {
    uint32_t planned[8];         // the plan this call goes by: its own (a call that waited) or the previous call's, scaled to this batch's size
    uint32_t last_count[8];      // final counts of the last finished call, scaled likewise
    uint32_t last_planned[8];    // what that call had planned
    uint64_t work[3];            // its wave-time in classes 0 - 2 (zeros: nothing measured)
    uint64_t measured_gw;        // ... and the lanes per group of class 0 it ran with
    bool valid;                  // a call of the same kind has been queued on this context before
};
// waited: the call has synchronised with its own plan (the first call of a context, a change of kind, HYPO_POA_SYNC_PLAN).  Otherwise
// the pinned block holds what the previous call left (complete unless that call is still running: then the one before it).
inline PoaHistory poa_history(const volatile PoaPinned* pinned, bool have_history, bool waited, const uint32_t prev_planned[8],
                              uint32_t n_windows, uint32_t history_windows) {
    PoaHistory h;
    const uint64_t num = waited ? 1 : n_windows, den = waited || !history_windows ? 1 : history_windows;
    for (int c = 0; c < 8; ++c) {
        h.planned[c] = (uint32_t)((uint64_t)pinned->plan[c] * num / den);
        h.last_count[c] = have_history ? (uint32_t)((uint64_t)pinned->final_count[c] * num / den) : 0u;
        h.last_planned[c] = !waited ? h.planned[c] : (have_history ? prev_planned[c] : 0u);
    }
    for (int c = 0; c < 3; ++c) h.work[c] = have_history ? pinned->work[c] : 0ull;
    h.measured_gw = pinned->work[kPinnedGeometrySlot];
    h.valid = have_history;
    return h;
}

// Windows re-queued into a class are only known on the device.  The grids of the mop-up passes and of the rare classes
// are sized from what the plan put there plus what the LAST finished call saw arrive later (its counters come back
// asynchronously at the end of every call): batches of one run look alike, and noisier reads re-queue many windows (at 1 %
// read error 3 % of the windows outgrow their class).  Without history a floor of a few hundred waves applies.
inline uint32_t late_arrivals(const PoaHistory& h, int cls, uint32_t n_windows) {
    const uint32_t seen = h.last_count[cls] > h.last_planned[cls] ? h.last_count[cls] - h.last_planned[cls] : 0u;
    // the mop-up passes of classes 1 and 2 are launched on the side streams, where the dispatch of idle waves (they leave
    // after one look at the queue) costs nothing: they get a generous floor.  Class 3 and later start on the caller's stream.
    // (a rare class the last finished call saw nothing of gets 32 waves instead of 256: a launch whose waves all leave at once costs 5 us
    // with 32 of them and 15-17 with 256, twice per call on the caller's stream = 1.3 % of the C2 step; waves are persistent, a surprise
    // is still drained, and the next call sizes for it)
    const uint32_t floor = cls < 3 ? (n_windows / 8 > 256 ? n_windows / 8 : 256) : ((h.valid && h.last_count[cls] == 0) ? 32u : 256u);
    const uint32_t want = seen + seen / 2 + floor;
    return want < n_windows ? want : n_windows;
}
inline uint32_t rare_grid_hint(const PoaHistory& h, int cls, uint32_t n_windows) {         // windows to size the grid of a rare class for
    const uint64_t want = (uint64_t)h.planned[cls] + late_arrivals(h, cls, n_windows);
    return (uint32_t)(want < n_windows ? want : n_windows);
}

// ------------------------------------------------------------------------------------------------
// wave shares of the three concurrent LDS-class kernels from the work of the last call
// ------------------------------------------------------------------------------------------------
// What a wave of a class takes of a CU: LDS bytes (granules of 512) and vector registers (granules of 8, 2 048 per CU).  The
// shares {w0, w1, w2} minimise max_c work[c] / w[c] under both budgets; the LDS budget is a CU's 160 KB plus the 5 % by which the
// measured-best fixed shares {5,5,6} overbook it (167 KB: the kernel submitted last grows into what the first one to run dry
// leaves), less what the polling class-3 waves hold.  Among shares within 3 % of the best the one with most waves wins (latency).
struct WaveFootprint { size_t lds; int vgprs; int max_waves; };
struct PoaFootprints { WaveFootprint c0, c0w, c1, c2, c3; uint64_t gw0, gw0w; };      // c0 / c0w: class 0 with four / two groups per wave, of gw0 / gw0w lanes
// something measured, and plausibly (not the first call, not a torn read: a wave lives < 10 s = 1e9 ticks, a launch has < 1e5 waves)
inline bool poa_work_plausible(const uint64_t work[3]) {
    if ((double)work[0] + (double)work[1] + (double)work[2] <= 0.0) return false;
    for (int c = 0; c < 3; ++c) if (work[c] > (uint64_t)1e14) return false;
    return true;
}
inline void pick_wave_shares(const uint64_t work[3], const WaveFootprint fp[3], const WaveFootprint& fp3, int poll_waves_per_cu, bool log, int caps[]) {
    if (!poa_work_plausible(work)) return;
    double lds_budget = 160.0 * 1024.0 * 1.05 - (double)poll_waves_per_cu * (double)fp3.lds;
    double vgpr_budget = 2048.0 - (double)poll_waves_per_cu * (double)fp3.vgprs * 0.5;      // (a polling wave sleeps most of the time, but it holds its registers)
    double best_t = 1e300; int best[3] = {caps[0], caps[1], caps[2]}, best_sum = 0;
    for (int pass = 0; pass < 2; ++pass) {                 // pass 0: the best time; pass 1: most waves within 3 % of it
        for (int w0 = 1; w0 <= fp[0].max_waves; ++w0)
            for (int w1 = 1; w1 <= fp[1].max_waves; ++w1)
                for (int w2 = 1; w2 <= fp[2].max_waves; ++w2) {
                    const double lds = (double)w0 * fp[0].lds + (double)w1 * fp[1].lds + (double)w2 * fp[2].lds;
                    const double vg = (double)w0 * fp[0].vgprs + (double)w1 * fp[1].vgprs + (double)w2 * fp[2].vgprs;
                    if (lds > lds_budget || vg > vgpr_budget) continue;
                    double t = (double)work[0] / w0;
                    if ((double)work[1] / w1 > t) t = (double)work[1] / w1;
                    if ((double)work[2] / w2 > t) t = (double)work[2] / w2;
                    if (pass == 0) { if (t < best_t) best_t = t; }
                    else if (t <= best_t * 1.03 && w0 + w1 + w2 > best_sum) { best_sum = w0 + w1 + w2; best[0] = w0; best[1] = w1; best[2] = w2; }
                }
        if (best_t >= 1e300) return;                       // nothing fits (cannot happen: {1,1,1} does)
    }
    caps[0] = best[0]; caps[1] = best[1]; caps[2] = best[2];
    if (log) fprintf(stderr, "[hypo_gpu] wave shares {%d,%d,%d} from wave-time {%.2f, %.2f, %.2f} ms (x 1 wave), poll %d\n",
                     caps[0], caps[1], caps[2], work[0] * 1e-5, work[1] * 1e-5, work[2] * 1e-5, poll_waves_per_cu);
}

// ------------------------------------------------------------------------------------------------
// the schedule of one call
// ------------------------------------------------------------------------------------------------
// The plan's class counts decide class 0's geometry and wave share and size the grids
// of the rare classes (3: oversized, 4: LONG, 5: catch-all): a grid of 2 048 single-wave workgroups costs ~0.1 ms of
// dispatch even if every wave leaves at once, and these classes are empty in most batches (a few escalated windows still
// find a small grid waiting).  An idle persistent wave exits after one failed dequeue, so grids may be generous.
struct PoaSchedule {
    bool sequential;             // one class kernel after the other on the caller's stream; the fields down to poll_cap are then unused
    bool four_groups;            // class 0 with four 16-lane groups per wave (else two 32-lane ones)
    int caps[3];                 // waves per CU of the three concurrent first passes
    char order[4];               // ... and the order they are submitted in
    bool long_first_pass;        // class 4's planned windows on a side stream next to the short-window kernels
    uint8_t main_class;          // the first pass (0 - 2) on the caller's stream; the other two on the side streams in class order
    uint32_t first4;             // ... that many
    uint32_t poll_waves;         // windows the polling launch of class 3 is sized for (0: no polling launch)
    int poll_cap;                // its waves per CU
    uint32_t hint3, hint4, hint5;// windows the regular launches of the rare classes are sized for
    uint32_t mopup4;             // ... and class 4's mop-up pass behind a first pass of its own
};
static_assert(sizeof(PoaSchedule) == 52 && offsetof(PoaSchedule, main_class) == 21 && offsetof(PoaSchedule, first4) == 24 && offsetof(PoaSchedule, mopup4) == 48,
              "main_class sits in the padding behind long_first_pass: tests/test_poa_schedule_cpu.py mirrors the struct field by field");
// The regular class-3 launch starts when classes 0 - 2 are done (the queue is final then) and does NOT wait for the polling launch's last
// window: the two drain the queue side by side (one cursor; the polling waves claim with a compare-and-swap below the count, the
// regular ones with a fetch-add that may run past it), each with direction-code slices of its own.  Behind the polling launch it
// started up to a millisecond late at 1 % read error (3.5-4.0 ms in most calls, 4.8-5.3 in a third of them).  When the scratch has
// no room for a second set of slices (tiny batches) it waits as before.  (A knob that forced the wait is gone.)
inline bool poa_side_by_side(int groups3, uint32_t poll_groups) { return poll_groups > 0 && groups3 - (int)poll_groups >= 64; }

inline PoaSchedule poa_schedule(const PoaHistory& h, uint32_t n_windows, int groups4, const PoaKnobs& k, const PoaFootprints& fp) {
    PoaSchedule s = {};
    s.main_class = 2;
    s.hint3 = rare_grid_hint(h, 3, n_windows); s.hint4 = rare_grid_hint(h, 4, n_windows); s.hint5 = rare_grid_hint(h, 5, n_windows);
    s.mopup4 = late_arrivals(h, 4, n_windows);
    // One kernel after the other instead: when the last call left more than a tenth of its windows to class 3 (read error of
    // several per cent) every kernel is long and fills the chip alone, and fixed LDS shares only leave the share of whichever
    // kernel ends first idle: 5 % read error 47 -> 40 ms, 3 % 30 -> 29 ms; below that the concurrent schedule wins (2 %: 20 against
    // 21.6 ms, C2: 3.7 against 4.2 ms; profiles/diag/r03_seq.sh, r03_backfill.sh).  HYPO_POA_SEQUENTIAL=0|1 forces.
    s.sequential = k.sequential >= 0 ? k.sequential > 0 : (h.valid && (uint64_t)h.last_count[3] * kSequentialDivisor > n_windows);
    if (s.sequential) return s;
    // The three LDS classes run CONCURRENTLY on the caller's stream and two auxiliary streams: the small-window
    // kernels are latency bound (most sequences reuse an alignment) while the large-window kernel saturates VALU
    // issue, so sharing the CUs fills issue slots either would leave idle (measured: ~11 % per step).  Each gets a
    // share of a CU's LDS through a waves-per-CU cap.  A window re-queued by a class that ran next to its successor
    // is picked up by a mop-up launch afterwards; the rare classes follow on the caller's stream.
    //
    // waves per CU of the three concurrent kernels (they share the CU's 160 KB of LDS, which is what bounds residency: 8 / 8 /
    // 14.5 KB per wave of classes 0 / 1 / 2 since class 1 runs one window per wave; 7.6 / 15.8 / 14.1 KB when the sweep below was made).  Caps whose footprints add up to about one CU's LDS make the split independent of
    // which kernel the dispatcher happens to serve first — with {5,5,5} (187 KB) the last one to arrive got what was left until
    // another finished, and which one that was depended on the stream -> hardware queue mapping of the process (C2 call 3.5 - 4.2 ms
    // for the same code).  Swept on C2 under two mappings (profiles/diag/caps_fit_sweep.sh, ms per call): {4,4,5} 3.48 / 3.48,
    // {3,4,5} 3.64 / 3.55, {4,3,5} 3.60 / 3.71, {4,4,4} 3.64 / 3.94, {5,5,5} 3.61 / 3.78, {5,4,4} 3.58 / 4.13.  Class 0 is set below.
    // After Poa::fetch_next and with class 1 at one window per wave (8 KB per wave): {5,5,6} (profiles/diag/r03_wave_wide_sweep2.sh:
    // C2 2.56 ms, 0.5 % read error 4.76, 1 % 10.2; {4,5,6} 2.56 / 4.72 / 11.1, {4,6,6} 2.65 / 4.96 / 11.3, {4,4,5} 2.94 / - / 9.8-11).
    // Round 5, after the one-substitution shortcut and Poa::topo_insert took a third off class 2's work: {5,5,5} (154.6 KB: every wave
    // resident, the three kernels' times stop swapping places between runs) — profiles/diag/r05_caps_fit.txt, ms per call at
    // 0.2 / 0.5 / 2 / 3 % read error: {5,5,6} 1.61-1.64 / 2.43-2.44 / 15.2-15.7 / 24.7-24.9, {5,5,5} 1.55 x 3 / 2.33 / 13.7-14.1 /
    // 22.5-22.6, {6,4,5} 1.56-1.59, {5,4,6} 1.55-1.69, {4,5,6} 1.61-1.66; 1 % alone prefers {5,5,6} (5.4-5.8 against 5.8-6.6).
    for (int c = 0; c < 3; ++c) s.caps[c] = k.caps[c];
    // The host looks at the plan before it launches anything: a batch made of tiny windows almost only (dense short reads
    // on a large genome) runs class 0 with twice the waves (the default split starves it: 44 -> 55 M windows/s there).
    const uint64_t lds_windows = (uint64_t)h.planned[0] + h.planned[1] + h.planned[2];
    s.four_groups = k.class0 >= 0 ? k.class0 == 16 : (uint64_t)h.planned[0] * 100 > lds_windows * 85;      // (HYPO_POA_CLASS0: tests)
    if (!k.caps_set && s.four_groups) { s.caps[0] = 7; s.caps[1] = 6; s.caps[2] = 5; }      // (dense shape: {7,6,5} 76.0 M windows/s, {8,5,4} 74.8, {7,4,5} 73.4)
    // ... and from the second call on, batches of tiny windows get their shares from the WORK of the last finished call
    // (pick_wave_shares: wave-time per class as the kernels measured it, shares that let the three end together within the
    // CU's LDS and registers): the mix of classes differs from genome to genome there (dense short reads: 91 % / 8 % / 1 % of
    // the windows -> {7,5,1}, 69.6 -> 76.9-77.5 M windows/s; HiFi-like 56.3 -> 59.3-59.8 M).  Mixed batches keep the fixed
    // shares: on the C2 batch the model's pick lost (0.2 % read error {4,4,7}: 2.57 -> 3.03 ms — class 2 issues VALU work back
    // to back and gains little from a seventh wave, class 0 ends with single long windows, not with a shortage of waves), and
    // from 1 % read error on the chip is full whatever the shares are: nine fixed splits, each run twice, all landed within
    // 10.0-11.1 ms at 1 % and 17.4-19.9 ms at 2 % while the three kernels' own times swapped places from run to run
    // (profiles/diag/r03_adapt_ab.sh, r03_caps_err_sweep.sh + .txt).  HYPO_POA_ADAPT=1 forces the model everywhere, 0 turns it off.
    const bool adapt = k.adapt >= 0 ? k.adapt != 0 : s.four_groups;
    // (the measurement must come from a call that ran class 0 in the geometry this call picks: the calls of a run are
    // queued without waiting for each other, so the last FINISHED call may be a batch of another kind, and a class-0 wave
    // of four groups takes twice the time of one of two)
    const bool same_kind = h.measured_gw == (s.four_groups ? fp.gw0 : fp.gw0w);
    if (!k.caps_set && adapt && h.valid && same_kind) {
        const uint32_t seen3_now = h.last_count[3] > h.planned[3] ? h.last_count[3] : h.planned[3];
        const int poll_waves_per_cu = seen3_now == 0 ? 0 : ((seen3_now + seen3_now / 4) > 512u ? 2 : 1);
        const WaveFootprint f[3] = {s.four_groups ? fp.c0 : fp.c0w, fp.c1, fp.c2};
        pick_wave_shares(h.work, f, fp.c3, poll_waves_per_cu, k.adapt_log, s.caps);
    }
    // (Experiment, tried and left out: a second class-2 launch behind class 0 / class 1 on their streams, to take over the LDS share those leave
    // when they end early.  profiles/r06_backfill.txt: non-i.i.d. batch 10.4 -> 10.1-10.2 ms, C2 1.33 -> 1.38-1.46 ms, 1-2 % read error
    // within noise — the waves that are resident already are what issue is shared between; more of them add little.)
    // Submission order decides who gets LDS first: class 2 and class 0 start with their full share, class 1 takes what is
    // left and grows when class 0 runs dry.  Measured on C2 (ms per call): 201 3.89, 021 4.28, 120 4.38, 210 4.69, 102 4.72,
    // 012 4.76 (HYPO_POA_ORDER, for experiments).
    memcpy(s.order, k.order, 4);
    // Which first pass rides the caller's stream (the other two take aux[0] and aux[1] in class order): everything behind the first passes
    // is queued there, so it follows that kernel as a dependency within one queue, and the caller's stream needs no fork, so that kernel
    // starts first.  It is the class with the strictly largest wave-time per wave of its share in the last finished call, if that call ran
    // class 0 in this call's geometry and its values are plausible.  Anything else, a tie included, leaves class 2 there (the assignment
    // until round 8).  HYPO_POA_MAIN=0|1|2 forces.  On the C2 batch the rule keeps class 2; class 0 forced there starts first, takes issue
    // slots from class 2 and the step is slower (1.469 against 1.371 ms: DESIGN.md 3.1, profiles/r08_c2_step_trace.txt).
    if (k.main_class >= 0) s.main_class = (uint8_t)k.main_class;
    else if (h.valid && same_kind && poa_work_plausible(h.work)) {
        double t[3];
        for (int c = 0; c < 3; ++c) t[c] = (double)h.work[c] / (double)(s.caps[c] < 1 ? 1 : s.caps[c]);
        if (t[0] > t[1] && t[0] > t[2]) s.main_class = 0;
        else if (t[1] > t[0] && t[1] > t[2]) s.main_class = 1;
    }
    // LONG windows are planned straight into class 4, so its first pass does not have to wait for
    // anybody: it runs on a third stream next to the short-window kernels (a LONG window occupies one wave for ~0.1 s; its
    // latency is the floor of the whole call), and only the few windows escalated into class 4 later wait for the mop-up
    // pass at the end.
    // (only while every LONG window of the batch gets a wave of its own: the kernel is then bound by the latency of its
    // windows and leaves room.  A batch with more LONG windows keeps the whole chip busy for many window lifetimes, and
    // running it next to the short-window kernels was measured slower than after them — C4 mix, 400 000 SHORT + 8 000 LONG
    // windows: 313 ms against 285 ms — once the two really overlapped, which depends on the process's hardware queues)
    s.long_first_pass = h.planned[4] > 0 && h.planned[4] <= (uint32_t)groups4;
    s.first4 = h.planned[4];
    // Class 3 (what outgrows class 2, and the wide SHORT windows) runs NEXT to the classes that feed it: a polling launch on a
    // stream of its own takes the windows the plan put there and every re-queued window as it arrives (with its graph, Poa::
    // spill), instead of starting when classes 0 - 2 are done — at 0.5 % read error ONE window re-queued into class 3 used to
    // run 2.7 ms on its own behind 5.2 ms of first passes.  It is submitted after every launch it waits for (see
    // poa_class_kernel), sized by what the plan and the last call's late arrivals say; HYPO_POA_POLL=0 turns it off.
    // The regular launch behind the join takes what is left (nothing, unless the polling pass was cut short).
    // A polling wave holds its 16 KB of LDS while it waits, and the launches it waits for must always find room: at most two
    // per CU (one unless the last call saw many windows in the class), and no polling launch at all when the history says the class
    // stays empty (HYPO_POA_POLL_WAVES overrides the count).
    // Waves of the polling launch: what the plan put into class 3 (known work: one wave per window and a quarter more) + what the last
    // call saw ARRIVE later.  A wave per expected arrival (rounds 3-5) cost the 1 % read-error point 3 of its 7 ms — 640 waves, two per CU, idling through a
    // call whose 514 late windows are 0.18 s of wave time — so up to 1 024 arrivals get an eighth of that (they are served as they come,
    // a few per wave, and the regular launch behind the join takes what is left), up to 2 048 a quarter (1.25 % / 1.5 %: 7.2 / 7.7 -> 5.7 / 6.7 ms);
    // beyond that the class has real work and keeps a wave per window (2 % read error: 8.2 ms against 10.1-10.5 with 64-256 waves).
    // profiles/r06_poll_waves.txt, whose RULE=0 rows are the old sizing (a wave and a quarter per window seen; gone).
    const uint32_t planned3 = h.planned[3], arrivals = h.last_count[3] > planned3 ? h.last_count[3] - planned3 : 0u;
    s.poll_waves = planned3 + planned3 / 4;
    // ... and none at all once more than about 3 % of the batch arrives late: the first-pass kernels then keep the chip busy for as long
    // as the late windows take anyway, and class 3 runs behind the join with every CU to itself (2.5 / 3 / 4 % read error: 11.9 / 15.4 /
    // 20.9 -> 10.8 / 12.9 / 17.0 ms; at 2 % read error, 3.0 % late, polling still wins: 8.4 against 9.0)
    const bool many_late = (uint64_t)arrivals * 32u > (uint64_t)n_windows;
    if (many_late) s.poll_waves = 0;                       // (what the plan put into class 3 waits for the join with the rest)
    if (arrivals && !many_late) s.poll_waves += arrivals <= 1024u ? (arrivals / 8 > 8u ? arrivals / 8 : 8u) : (arrivals <= 2048u ? arrivals / 4 : arrivals + arrivals / 4);
    s.poll_cap = s.poll_waves > 512u ? 2 : 1;
    if (k.caps_set && k.caps[3] > 0) s.poll_cap = k.caps[3];
    if (k.poll_waves_set) s.poll_waves = k.poll_waves;
    if (!k.poll) s.poll_waves = 0;                         // (none: no polling launch; the regular one still takes what turns up)
    return s;
}

// Waves of one launch.  occupancy: what the runtime says a CU holds of the kernel; cap: the schedule's share (0: none); clamp_groups:
// the class keeps per-group slices in HBM scratch (the HBM-scratch classes, Cfg::DIRG) and group_cap of them are this launch's.
inline long poa_grid(int occupancy, int knob_waves_per_cu, int cap, int num_cus, int groups_per_wave, bool clamp_groups, int group_cap, uint32_t n_windows) {
    int per_cu = occupancy < 1 ? 1 : occupancy;
    if (knob_waves_per_cu >= 1 && knob_waves_per_cu < per_cu) per_cu = knob_waves_per_cu;
    if (cap >= 1 && cap < per_cu) per_cu = cap;
    long grid = (long)per_cu * num_cus;
    if (clamp_groups && grid * groups_per_wave > group_cap) grid = group_cap / groups_per_wave;
    const long need = ((long)n_windows + groups_per_wave - 1) / groups_per_wave;      // never more waves than windows
    if (grid > need) grid = need;
    return grid < 1 ? 1 : grid;
}

}  // namespace hypo
