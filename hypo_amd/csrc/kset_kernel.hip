// kset_kernel.hip — an exact set of canonical k-mers, k = 12..31, as a hash table in HBM (hypo --qv: the k-mers of the short reads,
// queried with the draft and the polished contigs; DESIGN.md "k-mer QV").  The count table of kmer_kernel.hip is direct-address and
// stops at k = 17; this one is open addressing with linear probing over 64-bit slots.  The key is the canonical code min(fwd, rc)
// itself (A0 C1 G2 T3, MSB-first, 2k <= 62 bits), all-ones marks a free slot, the home slot is the high half of
// mix64(key) * slots (any number of slots, no modulo).  Keys are never removed or changed, so a slot goes from free to one key once.
//   * kset_insert_kernel: bytes staged through LDS and fwd / rc rolled per lane exactly as kmer_count_kernel does.  A lane LOADS its
//     slot first: the key is there already for all but the first occurrence of a k-mer (29 of 30 at 30x) and no atomic is issued.
//     Only a free slot gets a 64-bit compare-and-swap; a lane that loses it to another key goes on to the next slot, one that loses
//     it to its own key is done.  New keys are summed per wave and added to the table's counter once per wave.
//   * kset_rehash_kernel: the keys of an old table into a larger one, same probe.
//   * kset_query_kernel: lanes over the positions of n_seqs byte strings laid back to back; a k-mer never spans two of them.  A
//     lookup is a read-only probe that ends at the key or at a free slot.  Windows and misses are summed per wave and added per
//     sequence with one 64-bit add each (a lane whose stretch crosses into another sequence adds what it has first); the sums are
//     integers, so their order does not matter.
// Forward progress: every probe loop runs at most `slots` steps.  A lane of the insert or rehash kernel that finds neither its key
// nor a free slot sets the overflow flag and leaves; lanes in a long probe look at the flag every 64 steps and leave too.  The host
// keeps the table at most half full, so the flag says "internal error", but no input can make a kernel spin.
// Bounds: bytes [0, n) are read (LDS beyond n holds a separator), slot indices are < slots by construction, total / missing
// indices are < n_seqs (a lane's sequence comes from a search in off[0 .. n_seqs] for a position < n = off[n_seqs]).
#include <hip/hip_runtime.h>
#include "kset_kernel.hpp"

namespace hypo {

constexpr int KS_THREADS = 256;
constexpr int KS_STRETCH = 32;                                  // bytes whose k-mers one lane handles
constexpr int KS_BLOCK_BYTES = KS_THREADS * KS_STRETCH;         // 8 KiB per workgroup
constexpr int KS_HALO = 32;                                     // >= k - 1 for k <= 31, a multiple of 16

__device__ __forceinline__ uint32_t ks_base_code(uint32_t b) {   // 0..3 for ACGTacgt, 4 for every other byte
    const uint32_t l = b | 0x20u;
    return l == 'a' ? 0u : l == 'c' ? 1u : l == 'g' ? 2u : l == 't' ? 3u : 4u;
}

__device__ __forceinline__ uint64_t ks_mix64(uint64_t x) {      // the 64-bit finaliser of MurmurHash3 (public domain)
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return x;
}
__device__ __forceinline__ uint64_t ks_home(uint64_t key, uint64_t slots) { return __umul64hi(ks_mix64(key), slots); }

// 1 when the key was new.  ctr[1]: the overflow flag.
__device__ __forceinline__ uint32_t ks_insert(uint64_t* table, uint64_t slots, uint64_t key, unsigned long long* ctr) {
    uint64_t s = ks_home(key, slots);
    for (uint64_t probe = 0; probe < slots; ++probe) {
        const uint64_t cur = __hip_atomic_load(table + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == key) return 0;
        if (cur == KSET_EMPTY) {
            const uint64_t prev = atomicCAS((unsigned long long*)(table + s), (unsigned long long)KSET_EMPTY, (unsigned long long)key);
            if (prev == KSET_EMPTY) return 1;
            if (prev == key) return 0;                          // lost the race to a lane with the same k-mer
        }
        if (++s == slots) s = 0;
        if ((probe & 63) == 63 && __hip_atomic_load(ctr + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return 0;
    }
    atomicOr(ctr + 1, 1ull);
    return 0;
}

__device__ __forceinline__ bool ks_contains(const uint64_t* __restrict__ table, uint64_t slots, uint64_t key) {
    uint64_t s = ks_home(key, slots);
    for (uint64_t probe = 0; probe < slots; ++probe) {
        const uint64_t cur = table[s];
        if (cur == key) return true;
        if (cur == KSET_EMPTY) return false;
        if (++s == slots) s = 0;
    }
    return false;
}

// bytes [b0, b0 + KS_BLOCK_BYTES + KS_HALO) of the input into LDS with 16-byte loads; '\n' beyond n
__device__ __forceinline__ void ks_stage(uint8_t* sb, const uint8_t* __restrict__ bytes, uint64_t b0, uint64_t n) {
    for (int x = threadIdx.x * 16; x < KS_BLOCK_BYTES + KS_HALO; x += KS_THREADS * 16) {
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

__device__ __forceinline__ void ks_wave_add(unsigned long long* dst, uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(dst, (unsigned long long)v);
}

__global__ void __launch_bounds__(KS_THREADS) kset_insert_kernel(const uint8_t* __restrict__ bytes, uint64_t n, uint32_t k,
                                                                  uint64_t* table, uint64_t slots, unsigned long long* ctr) {
    __shared__ __attribute__((aligned(16))) uint8_t sb[KS_BLOCK_BYTES + KS_HALO];
    ks_stage(sb, bytes, (uint64_t)blockIdx.x * KS_BLOCK_BYTES, n);
    const uint64_t mask = (1ull << (2 * k)) - 1;
    const uint32_t rsh = 2 * (k - 1);
    const int s0 = threadIdx.x * KS_STRETCH;
    const int last = s0 + KS_STRETCH + (int)k - 1;              // exclusive end of the bytes this lane reads
    uint64_t fwd = 0, rc = 0;
    uint32_t run = 0, n_new = 0;
    for (int p = s0; p < last; ++p) {
        const uint32_t c = ks_base_code(sb[p]);
        if (c > 3) { run = 0; continue; }
        fwd = ((fwd << 2) | c) & mask;
        rc = (rc >> 2) | ((uint64_t)(3u - c) << rsh);
        if (++run >= k) n_new += ks_insert(table, slots, fwd < rc ? fwd : rc, ctr);   // starts at p - k + 1 >= s0
    }
    ks_wave_add(ctr, n_new);
}

__global__ void __launch_bounds__(KS_THREADS) kset_rehash_kernel(const uint64_t* __restrict__ old_table, uint64_t old_slots,
                                                                  uint64_t* table, uint64_t slots, unsigned long long* ctr) {
    uint32_t n_new = 0;
    const uint64_t stride = (uint64_t)gridDim.x * KS_THREADS;
    for (uint64_t i = (uint64_t)blockIdx.x * KS_THREADS + threadIdx.x; i < old_slots; i += stride) {
        const uint64_t key = old_table[i];
        if (key != KSET_EMPTY) n_new += ks_insert(table, slots, key, ctr);
    }
    ks_wave_add(ctr, n_new);
}

__global__ void __launch_bounds__(KS_THREADS) kset_query_kernel(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ off,
                                                                 uint32_t n_seqs, uint64_t n, uint32_t k, const uint64_t* __restrict__ table,
                                                                 uint64_t slots, unsigned long long* total, unsigned long long* missing) {
    __shared__ __attribute__((aligned(16))) uint8_t sb[KS_BLOCK_BYTES + KS_HALO];
    const uint64_t b0 = (uint64_t)blockIdx.x * KS_BLOCK_BYTES;
    ks_stage(sb, bytes, b0, n);
    const uint64_t mask = (1ull << (2 * k)) - 1;
    const uint32_t rsh = 2 * (k - 1);
    const int s0 = threadIdx.x * KS_STRETCH;
    const int last = s0 + KS_STRETCH + (int)k - 1;
    uint32_t seq = 0;
    uint64_t seq_end = 0;
    unsigned long long tot = 0, mis = 0;
    if (b0 + (uint64_t)s0 < n) {
        // the sequence that holds the lane's first byte: the last one that starts at or before it (empty ones before it are skipped)
        const uint64_t g0 = b0 + (uint64_t)s0;
        uint32_t lo = 1, hi = n_seqs;                           // first index in [1, n_seqs] with off[index] > g0 (off[n_seqs] = n > g0)
        while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (off[mid] > g0) hi = mid; else lo = mid + 1; }
        seq = lo - 1;
        seq_end = off[lo];
        uint64_t fwd = 0, rc = 0;
        uint32_t run = 0;
        for (int p = s0; p < last; ++p) {
            const uint64_t g = b0 + (uint64_t)p;
            if (g >= n) break;
            if (g == seq_end) {                                  // the next sequence starts here (g < n: there is one that holds g)
                if (tot) { atomicAdd(total + seq, tot); if (mis) atomicAdd(missing + seq, mis); }
                tot = mis = 0; run = 0;
                do { ++seq; seq_end = off[seq + 1]; } while (seq_end == g);
            }
            const uint32_t c = ks_base_code(sb[p]);
            if (c > 3) { run = 0; continue; }
            fwd = ((fwd << 2) | c) & mask;
            rc = (rc >> 2) | ((uint64_t)(3u - c) << rsh);
            if (++run >= k) { ++tot; if (!ks_contains(table, slots, fwd < rc ? fwd : rc)) ++mis; }
        }
    }
    // per wave: the lanes that ended in the sequence of the wave's first lane are summed and added once, the others add their own
    const uint32_t lead = __shfl(seq, 0);
    const bool same = seq == lead;
    unsigned long long t = same ? tot : 0, m = same ? mis : 0;
    for (int o = 32; o > 0; o >>= 1) { t += __shfl_xor(t, o); m += __shfl_xor(m, o); }
    if ((threadIdx.x & 63) == 0 && t) { atomicAdd(total + lead, t); if (m) atomicAdd(missing + lead, m); }
    if (!same && tot) { atomicAdd(total + seq, tot); if (mis) atomicAdd(missing + seq, mis); }
}

hipError_t kset_insert_run(const uint8_t* bytes, uint64_t n, uint32_t k, uint64_t* table, uint64_t slots, unsigned long long* ctr, hipStream_t st) {
    if (!n) return hipSuccess;
    const uint64_t blocks = (n + KS_BLOCK_BYTES - 1) / KS_BLOCK_BYTES;
    kset_insert_kernel<<<dim3((uint32_t)blocks), dim3(KS_THREADS), 0, st>>>(bytes, n, k, table, slots, ctr);
    return hipGetLastError();
}

hipError_t kset_rehash_run(const uint64_t* old_table, uint64_t old_slots, uint64_t* table, uint64_t slots, unsigned long long* ctr, hipStream_t st) {
    if (!old_slots) return hipSuccess;
    uint64_t blocks = (old_slots + KS_THREADS - 1) / KS_THREADS;
    if (blocks > 16384) blocks = 16384;
    kset_rehash_kernel<<<dim3((uint32_t)blocks), dim3(KS_THREADS), 0, st>>>(old_table, old_slots, table, slots, ctr);
    return hipGetLastError();
}

hipError_t kset_query_run(const uint8_t* bytes, const uint64_t* off, uint32_t n_seqs, uint64_t n, uint32_t k, const uint64_t* table,
                          uint64_t slots, unsigned long long* total, unsigned long long* missing, hipStream_t st) {
    if (!n || !n_seqs) return hipSuccess;
    const uint64_t blocks = (n + KS_BLOCK_BYTES - 1) / KS_BLOCK_BYTES;
    kset_query_kernel<<<dim3((uint32_t)blocks), dim3(KS_THREADS), 0, st>>>(bytes, off, n_seqs, n, k, table, slots, total, missing);
    return hipGetLastError();
}

}  // namespace hypo
