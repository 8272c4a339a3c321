// kmer_kernel.hip — the solid k-mer set built from the short reads on the device (replaces KMC run with -k<k> -ci2 -cs<4c>
// -cx<4c> and suk::SolidKmers::initialise, external/suk/src/SolidKmers.cpp:68-208).  Three kernels over one direct-address count
// table of 4^k counters, indexed by the canonical code min(fwd, rc) (A0 C1 G2 T3, MSB-first):
//   * kmer_count_kernel: staging and the per-lane rolling codes are those of kmer_roll.hpp; the lane counts the k-mers that START
//     in its stretch.  A counter is raised by a compare-and-swap loop on the dword that holds it, and never past
//     `sat` = 4c + 1 ("above -cx"): exact under any contention (a poly-A run raises one counter millions of times) and the carry of a
//     1- or 2-byte counter can never reach its neighbour.  A lane that reads a saturated counter issues no atomic at all.
//   * kmer_histogram_kernel: 16-byte reads of the table, per-workgroup bins in LDS, one 64-bit global add per non-zero bin and workgroup.
//   * solid_fill_kernel: a gather; each lane writes whole 64-bit words of the 4^k-bit set: for every code y of its word it reads
//     count[canon(y)] and applies the cut-offs and the homopolymer rule (symmetric under reverse complement), so both strands of a
//     solid canonical k-mer are set without atomics and the words are deterministic.  Popcounts of the words (all bits, and the bits
//     of canonical codes) are summed per wave and added once per wave.
// Bounds: the count kernel reads as kmer_roll.hpp says, table indices are < 4^k by construction (both codes are masked to 2k
// bits), the fill kernel writes words [0, 4^k / 64).
#include <hip/hip_runtime.h>
#include "kmer_kernel.hpp"
#include "kmer_roll.hpp"

namespace hypo {

constexpr int KH_THREADS = 256;
constexpr int KF_THREADS = 256;

// counter of code `c` += 1 unless it holds `sat` already.  Counters of 8 (wide = 0) or 16 bits inside 32-bit words.
template <int WIDE>
__device__ __forceinline__ void count_one(uint32_t* table32, uint64_t c, uint32_t sat) {
    constexpr uint32_t kBits = WIDE ? 16u : 8u, kMask = WIDE ? 0xffffu : 0xffu, kPer = 32u / kBits;
    uint32_t* w = table32 + (c / kPer);
    const uint32_t sh = (uint32_t)(c % kPer) * kBits;
    uint32_t old = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (((old >> sh) & kMask) < sat) {
        const uint32_t prev = atomicCAS(w, old, old + (1u << sh));
        if (prev == old) break;
        old = prev;
    }
}

template <int WIDE>
__global__ void __launch_bounds__(KR_THREADS) kmer_count_kernel(const uint8_t* __restrict__ bytes, uint64_t n, uint32_t k,
                                                                 uint32_t* __restrict__ table32, uint32_t sat) {
    __shared__ __attribute__((aligned(16))) uint8_t sb[KR_BLOCK_BYTES + KR_HALO];
    kmer_stage(sb, bytes, (uint64_t)blockIdx.x * KR_BLOCK_BYTES, n);
    const int s0 = threadIdx.x * KR_STRETCH;
    const int last = s0 + KR_STRETCH + (int)k - 1;              // exclusive end of the bytes this lane reads
    KmerRoll roll(k);
    for (int p = s0; p < last; ++p)
        if (roll.push(sb[p])) count_one<WIDE>(table32, roll.canon(), sat);             // starts at p - k + 1 >= s0
}

template <int WIDE>
__global__ void __launch_bounds__(KH_THREADS) kmer_histogram_kernel(const uint4* __restrict__ table, uint64_t n_vec, uint32_t n_bins,
                                                                     unsigned long long* __restrict__ hist) {
    extern __shared__ uint32_t bins[];
    for (uint32_t i = threadIdx.x; i < n_bins; i += KH_THREADS) bins[i] = 0;
    __syncthreads();
    constexpr uint32_t kBits = WIDE ? 16u : 8u, kMask = WIDE ? 0xffffu : 0xffu;
    for (uint64_t i = (uint64_t)blockIdx.x * KH_THREADS + threadIdx.x; i < n_vec; i += (uint64_t)gridDim.x * KH_THREADS) {
        const uint4 v = table[i];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (!w[j]) continue;
#pragma unroll
            for (uint32_t s = 0; s < 32; s += kBits) {
                const uint32_t c = (w[j] >> s) & kMask;
                if (c >= 2 && c < n_bins) atomicAdd(&bins[c], 1u);
            }
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n_bins; i += KH_THREADS)
        if (bins[i]) atomicAdd(&hist[i], (unsigned long long)bins[i]);
}

__device__ __forceinline__ uint64_t rev_comp(uint64_t y, uint32_t k, uint64_t mask) {
    uint64_t x = __builtin_bitreverse64(y ^ mask);                                       // complement, then reverse the bits
    x = ((x >> 1) & 0x5555555555555555ull) | ((x & 0x5555555555555555ull) << 1);        // ... and put each base's two bits back in order
    return x >> (64 - 2 * k);
}

template <int WIDE>
__global__ void __launch_bounds__(KF_THREADS) solid_fill_kernel(const void* __restrict__ table, uint32_t k, uint32_t lower, uint32_t upper,
                                                                 uint32_t sat, int exclude_hp, uint64_t* __restrict__ bits, uint64_t n_words,
                                                                 unsigned long long* __restrict__ counts) {
    const uint64_t mask = (1ull << (2 * k)) - 1;
    const uint32_t hi = 2 * (k - 1), hi2 = 2 * (k - 2);
    unsigned long long n_bits = 0, n_canon = 0;
    for (uint64_t w = (uint64_t)blockIdx.x * KF_THREADS + threadIdx.x; w < n_words; w += (uint64_t)gridDim.x * KF_THREADS) {
        uint64_t word = 0, canon_bits = 0;
        for (uint32_t j = 0; j < 64; ++j) {
            const uint64_t y = w * 64 + j;
            if (exclude_hp && ((((y >> hi) ^ (y >> hi2)) & 3) == 0 || ((y ^ (y >> 2)) & 3) == 0)) continue;
            const uint64_t r = rev_comp(y, k, mask);
            const uint64_t c = y < r ? y : r;
            const uint32_t cnt = WIDE ? (uint32_t)((const uint16_t*)table)[c] : (uint32_t)((const uint8_t*)table)[c];
            if (cnt >= 2 && cnt < sat && cnt >= lower && cnt <= upper) {
                word |= 1ull << j;
                if (y <= r) canon_bits |= 1ull << j;
            }
        }
        bits[w] = word;
        n_bits += (unsigned long long)__popcll(word);
        n_canon += (unsigned long long)__popcll(canon_bits);
    }
    for (int off = 32; off > 0; off >>= 1) {
        n_bits += __shfl_xor(n_bits, off);
        n_canon += __shfl_xor(n_canon, off);
    }
    if ((threadIdx.x & 63) == 0 && (n_bits || n_canon)) {
        atomicAdd(&counts[0], n_bits);
        atomicAdd(&counts[1], n_canon);
    }
}

hipError_t kmer_count_run(const uint8_t* bytes, uint64_t n, uint32_t k, void* table, int wide, uint32_t sat, hipStream_t st) {
    if (!n) return hipSuccess;
    const uint64_t blocks = (n + KR_BLOCK_BYTES - 1) / KR_BLOCK_BYTES;
    if (wide) kmer_count_kernel<1><<<dim3((uint32_t)blocks), dim3(KR_THREADS), 0, st>>>(bytes, n, k, (uint32_t*)table, sat);
    else kmer_count_kernel<0><<<dim3((uint32_t)blocks), dim3(KR_THREADS), 0, st>>>(bytes, n, k, (uint32_t*)table, sat);
    return hipGetLastError();
}

hipError_t kmer_histogram_run(const void* table, uint32_t k, int wide, uint32_t n_bins, unsigned long long* hist, hipStream_t st) {
    hipError_t e = hipMemsetAsync(hist, 0, (size_t)n_bins * 8, st);
    if (e != hipSuccess) return e;
    const uint64_t n_vec = ((1ull << (2 * k)) * (wide ? 2 : 1)) / 16;          // k >= 5: a whole number of 16-byte vectors
    uint64_t blocks = (n_vec + KH_THREADS - 1) / KH_THREADS;
    if (blocks > 4096) blocks = 4096;
    const size_t lds = (size_t)n_bins * 4;
    if (wide) kmer_histogram_kernel<1><<<dim3((uint32_t)blocks), dim3(KH_THREADS), lds, st>>>((const uint4*)table, n_vec, n_bins, hist);
    else kmer_histogram_kernel<0><<<dim3((uint32_t)blocks), dim3(KH_THREADS), lds, st>>>((const uint4*)table, n_vec, n_bins, hist);
    return hipGetLastError();
}

hipError_t solid_fill_run(const void* table, uint32_t k, int wide, uint32_t lower, uint32_t upper, uint32_t sat, int exclude_hp,
                          uint64_t* bits, unsigned long long* counts, hipStream_t st) {
    hipError_t e = hipMemsetAsync(counts, 0, 16, st);
    if (e != hipSuccess) return e;
    const uint64_t n_words = (1ull << (2 * k)) / 64;
    uint64_t blocks = (n_words + KF_THREADS - 1) / KF_THREADS;
    if (blocks > 16384) blocks = 16384;
    if (wide) solid_fill_kernel<1><<<dim3((uint32_t)blocks), dim3(KF_THREADS), 0, st>>>(table, k, lower, upper, sat, exclude_hp, bits, n_words, counts);
    else solid_fill_kernel<0><<<dim3((uint32_t)blocks), dim3(KF_THREADS), 0, st>>>(table, k, lower, upper, sat, exclude_hp, bits, n_words, counts);
    return hipGetLastError();
}

}  // namespace hypo
