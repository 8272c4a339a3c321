// edit_kernel.hip — the canonical unit-cost alignment of a draft span `a` (n bytes) against its polished text `b` (m bytes), for
// every replacement unit of a polishing run (hypo --vcf; the contract is in DESIGN.md "Edit scripts").
//   D(i,0) = i, D(0,j) = j, D(i,j) = min(D(i-1,j-1) + [a_i != b_j], D(i-1,j) + 1, D(i,j-1) + 1); the traceback from (n,m) takes
//   the first move that holds in the order diagonal ('=' / 'X'), up ('D'), left ('I').
// Every pair first loses its common suffix (exact: with equal last bytes D(n,m) = D(n-1,m-1) and the diagonal is taken first);
// a == b and pairs with an empty side need no DP.  The rest is swept by anti-diagonals t = i + j over a band of diagonals
// k = j - i.  Cells of one anti-diagonal all have k = t (mod 2), so a lane that owns the diagonal pair (K0 + 2l, K0 + 2l + 1)
// computes one cell per step: its own value from step t - 2 is the diagonal term, its own value from step t - 1 is one of the
// up / left terms and one neighbour lane's value from step t - 1 the other.  Every step keeps its 2-bit move codes as two 64-bit
// ballots (16 bytes per 64 cells).
//   * fast path (edit_pair_kernel): one wave per pair over 128 diagonals that contain [min(0,D), max(0,D)] (D = m - n), centred.
//     One cross-lane move per step.  The band is exact when it covers [min(0,D) - h, max(0,D) + h], h = (d_b - |D|) / 2, d_b the
//     banded distance: every path of cost <= d_b lies there, and so does every neighbour the traceback could take.  Move codes in
//     LDS when the pair needs at most EDIT_LDS_STEPS anti-diagonals (the pair's bytes are staged in LDS too), else in the caller's
//     scratch (the long list, a second launch).  A pair the band cannot decide goes to the wide list with its d_b.
//   * wide path (edit_wide_kernel): one 256-lane workgroup per pair; its band is [min(0,D) - h, max(0,D) + h], h = (d - |D|) / 2 for
//     the bound d it was sent with, so every path of cost <= d lies inside.  A pair the fast band decided against comes with its
//     d_b: exact in one pass.  A pair whose |D| exceeds the fast band first runs as a probe with h = EDIT_PROBE_H; if the probe's
//     distance does not pass the exactness test it runs again with that distance as its bound.  Lanes own diagonal slots
//     (several each when the band is wider than 512), the values of the band live in one array indexed by diagonal (LDS up to
//     EDIT_WIDE_LDS_DIAGS, the scratch beyond): a step writes the slots of its parity and reads the other parity's, so one
//     barrier per step separates them.
// The traceback runs on one lane.  It writes run-length ops backwards into the move storage it has already walked past (the
// storage holds one spare anti-diagonal, so the suffix run and every later run land above the codes still to be read), then
// reserves its place in the run pool with one atomic add and copies them.  A pool that is too small is detected by the caller
// (cursor > capacity) and the call is repeated with a larger pool.
// Bounds: byte reads stay in [a_off[p], a_off[p+1]) / [b_off[p], b_off[p+1]); move storage of a pair is (n + m + 2) anti-diagonals x
// groups x 16 bytes, all indices below that; pool writes only below pool_cap.
#include <hip/hip_runtime.h>
#include "edit_kernel.hpp"

namespace hypo {

constexpr int EDIT_INF = 1 << 29;
constexpr int EDIT_WAVES = 4;                       // waves per workgroup of the fast path

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Runs of the alignment, backwards, at area[top], area[top - 1], ...: the suffix run first, then the DP's runs from (n, m) back to
// (0, 0).  code(i, j) is the move code of cell (i, j), i, j > 0.  Returns the number of runs; they are at area[top - R + 1 .. top]
// in draft order.
template <class Code>
__device__ uint32_t edit_traceback(const Code& code, uint32_t n, uint32_t m, uint32_t sfx, uint32_t* area, uint64_t top) {
    uint32_t R = 0;
    if (sfx) area[top - R++] = (sfx << 2) | 0u;
    uint32_t i = n, j = m, cur = 4, len = 0;
    while (i | j) {
        const uint32_t op = i == 0 ? 3u : j == 0 ? 2u : code(i, j);
        if (op != cur) { if (len) area[top - R++] = (len << 2) | cur; cur = op; len = 0; }
        ++len;
        if (op < 2) { --i; --j; } else if (op == 2) --i; else --j;
    }
    if (len) area[top - R++] = (len << 2) | cur;
    return R;
}

__device__ __forceinline__ void edit_emit(const EditIO& io, uint32_t p, uint32_t d, const uint32_t* runs, uint32_t R) {
    const unsigned long long start = atomicAdd(&io.counters[0], (unsigned long long)R);
    if (start + R <= io.pool_cap)
        for (uint32_t r = 0; r < R; ++r) io.pool[start + r] = runs[r];
    io.rstart[p] = (uint32_t)start; io.rcount[p] = R; io.dist[p] = d;
}

// common suffix of a[0, n) and b[0, m), by the whole wave
__device__ __forceinline__ uint32_t edit_suffix(const char* a, uint32_t n, const char* b, uint32_t m, int lane) {
    const uint32_t mn = n < m ? n : m;
    for (uint32_t c = 0; c < mn; c += 64) {
        const uint32_t q = c + (uint32_t)lane;
        const bool diff = q < mn ? a[n - 1 - q] != b[m - 1 - q] : true;
        const uint64_t bm = __ballot(diff);
        if (bm) return c + (uint32_t)__ffsll((unsigned long long)bm) - 1;
    }
    return mn;
}

// Banded sweep of one trimmed pair by one wave (A, B: its bytes, in LDS or global memory; mv: 2 words per anti-diagonal).
// Returns the banded distance and whether the band is exact for it.
__device__ uint32_t edit_band_sweep(const char* A, uint32_t n, const char* B, uint32_t m, int K0, uint64_t* mv, int lane, bool& exact) {
    int v1 = EDIT_INF, v2 = EDIT_INF;
    const uint32_t T = n + m;
    for (uint32_t t = 0; t <= T; ++t) {
        const int par = ((int)t + K0) & 1;
        const int k = K0 + 2 * lane + par;
        const int nb = par ? __shfl_down(v1, 1) : __shfl_up(v1, 1);
        int up, left;
        if (par) { left = v1; up = lane == 63 ? EDIT_INF : nb; }
        else { up = v1; left = lane == 0 ? EDIT_INF : nb; }
        const int ti = (int)t - k, tj = (int)t + k;
        int v = EDIT_INF; uint32_t c = 0;
        if (ti >= 0 && tj >= 0) {
            const int i = ti >> 1, j = tj >> 1;
            if (i <= (int)n && j <= (int)m) {
                if (i == 0) { v = j; c = 3; }
                else if (j == 0) { v = i; c = 2; }
                else {
                    const uint32_t x = A[i - 1] != B[j - 1];
                    const int dg = v2 + (int)x, u = up + 1, le = left + 1;
                    v = min(dg, min(u, le));
                    c = v == dg ? x : v == u ? 2u : 3u;
                }
            }
        }
        const uint64_t blo = __ballot(c & 1u), bhi = __ballot(c >> 1);
        if (lane == 0) { mv[2 * t] = blo; mv[2 * t + 1] = bhi; }
        v2 = v1; v1 = v;
    }
    const int delta = (int)m - (int)n, ad = delta < 0 ? -delta : delta;
    const int lend = (delta - K0 - ((int)(T + K0) & 1)) >> 1;
    const int d = __shfl(v1, lend);
    const int h = (d - ad) / 2;
    const int lo_req = max(-(int)n, min(0, delta) - h), hi_req = min((int)m, max(0, delta) + h);
    exact = lo_req >= K0 && hi_req <= K0 + (int)EDIT_FAST_BAND - 1;
    return (uint32_t)d;
}

__device__ __forceinline__ int edit_fast_k0(uint32_t n, uint32_t m) {
    const int delta = (int)m - (int)n, ad = delta < 0 ? -delta : delta;
    int K0 = min(0, delta) - ((int)EDIT_FAST_BAND - 1 - ad) / 2;
    if (K0 < -(int)n) K0 = -(int)n;
    else if (K0 + (int)EDIT_FAST_BAND - 1 > (int)m) K0 = max(-(int)n, (int)m - (int)EDIT_FAST_BAND + 1);
    return K0;
}

// LIST = 0: pairs [0, n_pairs), grid-stride by wave, moves and bytes in LDS (pairs that do not fit go to the long list).
// LIST = 1: entries [0, n_list) of the long list, moves at moves + moves_off[e], bytes read from global memory.
template <int LIST>
__global__ __launch_bounds__(EDIT_WAVES * 64) void edit_pair_kernel(EditIO io, const uint4* list, uint32_t n_list, uint8_t* moves,
                                                                    const uint64_t* moves_off) {
    __shared__ uint64_t lds_mv[LIST ? 1 : EDIT_WAVES][LIST ? 2 : 2 * EDIT_LDS_STEPS];
    __shared__ char lds_ab[LIST ? 1 : EDIT_WAVES][LIST ? 4 : EDIT_LDS_STEPS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t n_items = LIST ? n_list : io.n_pairs;
    const uint32_t stride = gridDim.x * EDIT_WAVES;
    for (uint32_t w = blockIdx.x * EDIT_WAVES + wave; w < n_items; w += stride) {
        const uint32_t p = LIST ? list[w].x : w;
        const char* a = io.a + io.a_off[p];
        const char* b = io.b + io.b_off[p];
        const uint32_t n0 = (uint32_t)(io.a_off[p + 1] - io.a_off[p]), m0 = (uint32_t)(io.b_off[p + 1] - io.b_off[p]);
        const uint32_t sfx = LIST ? list[w].y : edit_suffix(a, n0, b, m0, lane);
        const uint32_t n = n0 - sfx, m = m0 - sfx;
        if (!LIST && (n == 0 || m == 0)) {                  // a == b, or one side (after the suffix) empty: no DP
            if (lane == 0) {
                uint32_t runs[3], R = 0;
                if (n) runs[R++] = (n << 2) | 2u;
                if (m) runs[R++] = (m << 2) | 3u;
                if (sfx) runs[R++] = (sfx << 2) | 0u;
                edit_emit(io, p, n + m, runs, R);
            }
            continue;
        }
        const int delta = (int)m - (int)n, ad = delta < 0 ? -delta : delta;
        if (!LIST && ad > (int)EDIT_FAST_BAND - 1) {       // the band cannot hold both corners: a probe of the wide path
            if (lane == 0) { const uint32_t at = (uint32_t)atomicAdd(&io.counters[2], 1ull); io.wide_list[at] = make_uint4(p, sfx, (uint32_t)ad + 2 * EDIT_PROBE_H, 1u); }
            continue;
        }
        if (!LIST && n + m + 2 > EDIT_LDS_STEPS) {         // moves do not fit in LDS: the long list
            if (lane == 0) { const uint32_t at = (uint32_t)atomicAdd(&io.counters[1], 1ull); io.long_list[at] = make_uint4(p, sfx, 0u, 0u); }
            continue;
        }
        uint64_t* mv;
        const char *A = a, *B = b;
        if (LIST) mv = (uint64_t*)(moves + moves_off[w]);
        else {
            mv = lds_mv[LIST ? 0 : wave];
            char* s = lds_ab[LIST ? 0 : wave];
            for (uint32_t q = (uint32_t)lane; q < n + m; q += 64) s[q] = q < n ? a[q] : b[q - n];
            wave_sync();
            A = s; B = s + n;
        }
        const int K0 = edit_fast_k0(n, m);
        bool exact = false;
        const uint32_t d = edit_band_sweep(A, n, B, m, K0, mv, lane, exact);
        if (!exact) {
            if (lane == 0) { const uint32_t at = (uint32_t)atomicAdd(&io.counters[2], 1ull); io.wide_list[at] = make_uint4(p, sfx, d, 0u); }
            wave_sync();
            continue;
        }
        if (lane == 0) {
            auto code = [&](uint32_t i, uint32_t j) -> uint32_t {
                const uint32_t t = i + j;
                const int k = (int)j - (int)i, par = ((int)t + K0) & 1, l = (k - K0 - par) >> 1;
                return (uint32_t)((mv[2 * t] >> l) & 1u) | (uint32_t)(((mv[2 * t + 1] >> l) & 1u) << 1);
            };
            uint32_t* area = (uint32_t*)mv;
            const uint64_t top = 4ull * (n + m + 2) - 1;
            const uint32_t R = edit_traceback(code, n, m, sfx, area, top);
            edit_emit(io, p, d, area + (top + 1 - R), R);
        }
        wave_sync();
    }
}

__global__ __launch_bounds__(EDIT_WIDE_THREADS) void edit_wide_kernel(EditIO io, const uint4* list, uint8_t* moves, const uint64_t* moves_off,
                                                                      int32_t* vals, const uint64_t* vals_off) {
    __shared__ int32_t lds_v[EDIT_WIDE_LDS_DIAGS];
    const uint32_t e = blockIdx.x;
    const uint4 ent = list[e];
    const uint32_t p = ent.x, sfx = ent.y;
    const char* A = io.a + io.a_off[p];
    const char* B = io.b + io.b_off[p];
    const uint32_t n = (uint32_t)(io.a_off[p + 1] - io.a_off[p]) - sfx, m = (uint32_t)(io.b_off[p + 1] - io.b_off[p]) - sfx;
    int64_t lo64, hi64;
    edit_wide_band(n, m, ent.z, lo64, hi64);
    const int lo = (int)lo64, hi = (int)hi64;
    const uint32_t W = (uint32_t)(hi - lo + 1), S = (W + 1) / 2;
    const uint32_t G = (uint32_t)edit_wide_groups(lo64, hi64), C = (S + EDIT_WIDE_THREADS - 1) / EDIT_WIDE_THREADS;
    int32_t* V = W <= EDIT_WIDE_LDS_DIAGS ? lds_v : vals + vals_off[e];
    uint64_t* mv = (uint64_t*)(moves + moves_off[e]);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (uint32_t q = (uint32_t)tid; q < W; q += EDIT_WIDE_THREADS) V[q] = EDIT_INF;
    __syncthreads();
    const uint32_t T = n + m;
    for (uint32_t t = 0; t <= T; ++t) {
        const int par = ((int)t + lo) & 1;
        for (uint32_t c = 0; c < C; ++c) {
            const uint32_t s = c * EDIT_WIDE_THREADS + (uint32_t)tid;
            const int k = lo + 2 * (int)s + par;
            uint32_t code = 0;
            if (s < S && k <= hi) {
                const int ti = (int)t - k, tj = (int)t + k;
                int v = EDIT_INF;
                if (ti >= 0 && tj >= 0 && (ti >> 1) <= (int)n && (tj >> 1) <= (int)m) {
                    const int i = ti >> 1, j = tj >> 1;
                    if (i == 0) { v = j; code = 3; }
                    else if (j == 0) { v = i; code = 2; }
                    else {
                        const uint32_t x = A[i - 1] != B[j - 1];
                        const int dg = V[k - lo] + (int)x;
                        const int u = (k + 1 <= hi ? V[k + 1 - lo] : EDIT_INF) + 1;
                        const int le = (k - 1 >= lo ? V[k - 1 - lo] : EDIT_INF) + 1;
                        v = min(dg, min(u, le));
                        code = v == dg ? x : v == u ? 2u : 3u;
                    }
                }
                V[k - lo] = v;
            }
            const uint64_t blo = __ballot(code & 1u), bhi = __ballot(code >> 1);
            const uint32_t g = c * (EDIT_WIDE_THREADS / 64) + (uint32_t)wave;
            if (lane == 0 && g < G) { mv[2 * ((uint64_t)t * G + g)] = blo; mv[2 * ((uint64_t)t * G + g) + 1] = bhi; }
        }
        __syncthreads();
    }
    const int d_band = V[(int)m - (int)n - lo];
    if (ent.w) {                                            // a probe: its result stands only if the band is exact for it
        const int delta = (int)m - (int)n, ad = delta < 0 ? -delta : delta, h = (d_band - ad) / 2;
        const int lo_req = max(-(int)n, min(0, delta) - h), hi_req = min((int)m, max(0, delta) + h);
        if (lo_req < lo || hi_req > hi) {
            if (tid == 0) { const uint32_t at = (uint32_t)atomicAdd(&io.counters[3], 1ull); io.wide_list2[at] = make_uint4(p, sfx, (uint32_t)d_band, 0u); }
            return;
        }
    }
    if (tid == 0) {
        const uint32_t d = (uint32_t)d_band;
        auto code = [&](uint32_t i, uint32_t j) -> uint32_t {
            const uint32_t t = i + j;
            const int k = (int)j - (int)i, par = ((int)t + lo) & 1, s = (k - lo - par) >> 1;
            const uint64_t at = 2 * ((uint64_t)t * G + (uint32_t)(s >> 6));
            return (uint32_t)((mv[at] >> (s & 63)) & 1u) | (uint32_t)(((mv[at + 1] >> (s & 63)) & 1u) << 1);
        };
        uint32_t* area = (uint32_t*)mv;
        const uint64_t top = 4ull * G * (n + m + 2) - 1;
        const uint32_t R = edit_traceback(code, n, m, sfx, area, top);
        edit_emit(io, p, d, area + (top + 1 - R), R);
    }
}

hipError_t edit_fast_run(const EditIO& io, int num_cus, hipStream_t st) {
    if (!io.n_pairs) return hipSuccess;
    const uint32_t want = (io.n_pairs + EDIT_WAVES - 1) / EDIT_WAVES, cap = (uint32_t)(num_cus > 0 ? num_cus : 256) * 16;
    edit_pair_kernel<0><<<dim3(want < cap ? want : cap), dim3(EDIT_WAVES * 64), 0, st>>>(io, nullptr, 0, nullptr, nullptr);
    return hipGetLastError();
}

hipError_t edit_long_run(const EditIO& io, const uint4* list, uint32_t n, uint8_t* moves, const uint64_t* moves_off, hipStream_t st) {
    if (!n) return hipSuccess;
    edit_pair_kernel<1><<<dim3((n + EDIT_WAVES - 1) / EDIT_WAVES), dim3(EDIT_WAVES * 64), 0, st>>>(io, list, n, moves, moves_off);
    return hipGetLastError();
}

hipError_t edit_wide_run(const EditIO& io, const uint4* list, uint32_t n, uint8_t* moves, const uint64_t* moves_off, int32_t* vals,
                         const uint64_t* vals_off, hipStream_t st) {
    if (!n) return hipSuccess;
    edit_wide_kernel<<<dim3(n), dim3(EDIT_WIDE_THREADS), 0, st>>>(io, list, moves, moves_off, vals, vals_off);
    return hipGetLastError();
}

}  // namespace hypo
