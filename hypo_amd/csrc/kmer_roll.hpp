// kmer_roll.hpp — what the kernels that walk sequence bytes k-mer by k-mer share (device only): kmer_count_kernel of
// kmer_kernel.hip, kset_insert_kernel and the query / track-flags body of kset_kernel.hip.
//   * A 256-lane workgroup stages 8 KiB of sequence bytes (+ 32 bytes behind them) into LDS with 16-byte loads (kmer_stage).
//   * Every lane rolls the forward and reverse-complement codes (A0 C1 G2 T3, MSB-first, 2k bits) over its 32-byte stretch (+ k - 1
//     bytes of the next one) and handles the k-mers that START in its stretch, so every k-mer of the input is handled once
//     (KmerRoll).  Any byte other than ACGTacgt (N, IUPAC, the record separator) restarts the run.
// Bounds: bytes [0, n) are read (LDS beyond n holds a separator); a lane reads LDS bytes [s0, s0 + KR_STRETCH + k - 1) of its
// stretch at s0 = 32 * lane, which ends inside the staged KR_BLOCK_BYTES + KR_HALO bytes because k - 1 <= KR_HALO.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace hypo {

constexpr int KR_THREADS = 256;
constexpr int KR_STRETCH = 32;                                  // bytes whose k-mers one lane handles
constexpr int KR_BLOCK_BYTES = KR_THREADS * KR_STRETCH;         // 8 KiB per workgroup
constexpr int KR_HALO = 32;                                     // >= k - 1 for k <= 31, a multiple of 16

// 0..3 for ACGTacgt, 4 for every other byte (b | 0x20 folds the case and nothing else onto 'a', 'c', 'g', 't')
__device__ __forceinline__ uint32_t base_code(uint32_t b) {
    const uint32_t l = b | 0x20u;
    return l == 'a' ? 0u : l == 'c' ? 1u : l == 'g' ? 2u : l == 't' ? 3u : 4u;
}

// bytes [b0, b0 + KR_BLOCK_BYTES + KR_HALO) of the input into LDS with 16-byte loads; '\n' beyond n
__device__ __forceinline__ void kmer_stage(uint8_t* sb, const uint8_t* __restrict__ bytes, uint64_t b0, uint64_t n) {
    for (int x = threadIdx.x * 16; x < KR_BLOCK_BYTES + KR_HALO; x += KR_THREADS * 16) {
        const uint64_t g = b0 + (uint64_t)x;
        uint4 v;
        if (g + 16 <= n) {
            v = *(const uint4*)(bytes + g);                     // (g is a multiple of 16 and the buffer 256-byte aligned)
        } else {
            uint8_t tmp[16];
            for (int i = 0; i < 16; ++i) tmp[i] = g + i < n ? bytes[g + i] : (uint8_t)'\n';
            v = *(const uint4*)tmp;
        }
        *(uint4*)(sb + x) = v;
    }
    __syncthreads();
}

// The rolling codes of the last k bases a lane has pushed, k = 5..31 (2k <= 62 bits, so the mask is a plain shift).
struct KmerRoll {
    uint64_t mask, fwd = 0, rc = 0;
    uint32_t k, rsh, run = 0;
    __device__ __forceinline__ explicit KmerRoll(uint32_t k_) : mask((1ull << (2 * k_)) - 1), k(k_), rsh(2 * (k_ - 1)) {}
    __device__ __forceinline__ void reset() { run = 0; }       // the next window starts with the next byte
    __device__ __forceinline__ bool push(uint32_t byte) {       // true: a full window ends at this byte
        const uint32_t c = base_code(byte);
        if (c > 3) { run = 0; return false; }
        fwd = ((fwd << 2) | c) & mask;
        rc = (rc >> 2) | ((uint64_t)(3u - c) << rsh);
        return ++run >= k;
    }
    __device__ __forceinline__ uint64_t canon() const { return fwd < rc ? fwd : rc; }
};

}  // namespace hypo
