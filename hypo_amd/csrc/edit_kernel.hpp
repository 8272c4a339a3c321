// edit_kernel.hpp — host-visible interface of edit_kernel.hip (internal to libhypo_gpu.so): the canonical unit-cost alignment of
// every replaced draft span against its polished text (hypo --vcf; DESIGN.md "Edit scripts").
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hypo {

constexpr uint32_t EDIT_LDS_STEPS = 512;       // anti-diagonals whose move codes a wave keeps in LDS (fast path, LDS form)
constexpr uint32_t EDIT_FAST_BAND = 128;       // diagonals one wave covers (64 lanes x 2 parities)
constexpr uint32_t EDIT_WIDE_THREADS = 256;
constexpr uint32_t EDIT_WIDE_LDS_DIAGS = 8192; // wide path: the band's values in LDS up to this width, in the scratch beyond it

constexpr uint32_t EDIT_PROBE_H = 64;          // wide path, first pass of a pair the fast band cannot hold: h of the band
// Counters of one call (device memory, zeroed by the caller): [0] run-pool cursor, [1] entries of the long list, [2] of the wide
// list, [3] of the second wide list (pairs whose probe band was not exact).
struct EditIO {
    const char* a; const uint64_t* a_off; const char* b; const uint64_t* b_off; uint32_t n_pairs;
    uint32_t* dist; uint32_t* rstart; uint32_t* rcount;      // per pair: distance, where its runs are in the pool, how many
    uint32_t* pool; uint64_t pool_cap;                        // run-length ops, (len << 2) | op
    unsigned long long* counters;
    // entries {pair, suffix, distance bound, probe}: probe = 1 — the bound is |m - n| + 2 EDIT_PROBE_H, a first pass whose result
    // stands only if the band is exact for it; a pair it cannot decide goes to wide_list2 with the distance it found
    uint4* long_list; uint4* wide_list; uint4* wide_list2;
};

// Every pair: suffix trim, shortcuts, banded DP when the trimmed pair fits EDIT_LDS_STEPS; a pair that does not goes to the long
// list, a pair the band cannot decide to the wide list.
hipError_t edit_fast_run(const EditIO& io, int num_cus, hipStream_t st);
// entries [0, n) of the long list, move codes at moves + moves_off[e] (16 bytes per anti-diagonal)
hipError_t edit_long_run(const EditIO& io, const uint4* list, uint32_t n, uint8_t* moves, const uint64_t* moves_off, hipStream_t st);
// entries [0, n) of a wide list: one workgroup each; moves + moves_off[e], the band's values at vals + vals_off[e] when wider
// than EDIT_WIDE_LDS_DIAGS
hipError_t edit_wide_run(const EditIO& io, const uint4* list, uint32_t n, uint8_t* moves, const uint64_t* moves_off, int32_t* vals,
                         const uint64_t* vals_off, hipStream_t st);

// the wide band of a pair (host and device agree on it): diagonals [lo, hi] of the trimmed n x m problem with a distance bound d
__host__ __device__ inline void edit_wide_band(uint32_t n, uint32_t m, uint32_t d, int64_t& lo, int64_t& hi) {
    const int64_t delta = (int64_t)m - (int64_t)n, ad = delta < 0 ? -delta : delta;
    const int64_t h = ((int64_t)d - ad) / 2;
    lo = (delta < 0 ? delta : 0) - h; hi = (delta > 0 ? delta : 0) + h;
    if (lo < -(int64_t)n) lo = -(int64_t)n;
    if (hi > (int64_t)m) hi = (int64_t)m;
}
__host__ __device__ inline uint64_t edit_wide_groups(int64_t lo, int64_t hi) { return ((uint64_t)(hi - lo + 2) / 2 + 63) / 64; }

}  // namespace hypo
