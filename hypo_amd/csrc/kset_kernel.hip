// kset_kernel.hip — an exact set of canonical k-mers, k = 12..31, as a hash table in HBM (hypo --qv: the k-mers of the short reads,
// queried with the draft and the polished contigs; DESIGN.md "k-mer QV").  The count table of kmer_kernel.hip is direct-address and
// stops at k = 17; this one is open addressing with linear probing over 64-bit slots.  The key is the canonical code min(fwd, rc)
// itself (A0 C1 G2 T3, MSB-first, 2k <= 62 bits), all-ones marks a free slot, the home slot is the high half of
// mix64(key) * slots (any number of slots, no modulo).  Keys are never removed or changed, so a slot goes from free to one key once.
//   * kset_insert_kernel: bytes staged through LDS and fwd / rc rolled per lane by kmer_roll.hpp, as in kmer_count_kernel.  A lane LOADS its
//     slot first: the key is there already for all but the first occurrence of a k-mer (29 of 30 at 30x) and no atomic is issued.
//     Only a free slot gets a 64-bit compare-and-swap; a lane that loses it to another key goes on to the next slot, one that loses
//     it to its own key is done.  New keys are summed per wave and added to the table's counter once per wave.
//   * kset_rehash_kernel: the keys of an old table into a larger one, same probe.
//   * kset_query_kernel: lanes over the positions of n_seqs byte strings laid back to back; a k-mer never spans two of them.  A
//     lookup is a read-only probe that ends at the key or at a free slot.  Windows and misses are summed per wave and added per
//     sequence with one 64-bit add each (a lane whose stretch crosses into another sequence adds what it has first); the sums are
//     integers, so their order does not matter.
//   * kset_track_*_kernel (below, with comments of their own): the query kernel keeping its per-window answers as bit flags, and the
//     passes that turn the flags into sorted intervals of missing k-mers.
//   * kset_spans_kernel / kset_variants_kernel (below, with comments of their own): many short spans, and every subset of a few
//     edits of many short sites, a group of 32 or 64 lanes per item; read-only probes, no LDS, no atomics.  Both are ks_group_scan
//     with another source of bytes.
//   * kset_fixes_kernel / kset_fixes_reduce_kernel (below, with comments of their own; hypo --kmer-fix): every one-base edit of many
//     short regions, a group per candidate, ks_group_scan once more, and a lane per site that picks the best candidate.
//   * kset_walks_kernel (below, with comments of its own; hypo --kmer-bridge): the set as a de Bruijn graph, a depth-first search
//     between two anchors per site, 4 lanes a site, dependent probes, the stack in LDS.
//   * kset_walk_sets_kernel (below, with comments of its own; hypo --kmer-bridge-vote): that search carried on to up to four walks,
//     each with the least count byte along it.
//   * counts (hypo --qv-spectra; further down, with comments of their own): a count byte and up to four copy bytes per slot in planes
//     beside the table, a saturating byte add that serves both, and the counted variants of the insert and rehash kernels, the mark
//     kernel (the query body with a probe that returns the slot) and the spectrum kernel.
//   * a least count (hypo --qv-min-count; further down, with comments of their own): the query, track-flags, spans and variants
//     kernels once more as kset_*_min_kernel, whose probe also loads the hit slot's count byte and answers "seen at least t times".
//     They are instances of the same bodies with a compile-time switch; the kernels above do not know of t.
//   * export and import (hypo --qv-save / --qv-load; at the end, with comments of their own): the table's records out in slot order
//     by a stream compaction, and records back in with a saturating add of their count bytes.
//   * depth (hypo --qv-cn; at the end, with comments of its own): per bin of a text the read count byte of every window against its
//     copy byte, a wave per bin, a histogram of the count bytes in LDS for the median.
// Forward progress: every probe loop runs at most `slots` steps.  A lane of the insert or rehash kernel that finds neither its key
// nor a free slot sets the overflow flag and leaves; lanes in a long probe look at the flag every 64 steps and leave too.  The host
// keeps the table at most half full, so the flag says "internal error", but no input can make a kernel spin.
// Bounds: bytes are read as kmer_roll.hpp says, slot indices are < slots by construction, total / missing indices are < n_seqs
// (a lane's sequence comes from ks_seq_of, a search in off[0 .. n_seqs] for a position < n = off[n_seqs]).
#include <hip/hip_runtime.h>
#include <type_traits>
#include "kset_kernel.hpp"
#include "kmer_roll.hpp"

namespace hypo {

static_assert(KS_THREADS == KR_THREADS, "every kernel of this file has the workgroup of kmer_roll.hpp");

__device__ __forceinline__ uint64_t ks_mix64(uint64_t x) {      // the 64-bit finaliser of MurmurHash3 (public domain)
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return x;
}
__device__ __forceinline__ uint64_t ks_home(uint64_t key, uint64_t slots) { return __umul64hi(ks_mix64(key), slots); }

// 1 when the key was new.  ctr[1]: the overflow flag.  AT (the counted kernels): *at = the key's slot, found or claimed, and
// KSET_EMPTY for a lane that leaves without one (the overflow flag is then set).
template <bool AT = false>
__device__ __forceinline__ uint32_t ks_insert(uint64_t* table, uint64_t slots, uint64_t key, unsigned long long* ctr, uint64_t* at = nullptr) {
    uint64_t s = ks_home(key, slots);
    if (AT) *at = KSET_EMPTY;
    for (uint64_t probe = 0; probe < slots; ++probe) {
        const uint64_t cur = __hip_atomic_load(table + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == key) { if (AT) *at = s; return 0; }
        if (cur == KSET_EMPTY) {
            const uint64_t prev = atomicCAS((unsigned long long*)(table + s), (unsigned long long)KSET_EMPTY, (unsigned long long)key);
            if (prev == KSET_EMPTY) { if (AT) *at = s; return 1; }
            if (prev == key) { if (AT) *at = s; return 0; }     // lost the race to a lane with the same k-mer
        }
        if (++s == slots) s = 0;
        if ((probe & 63) == 63 && __hip_atomic_load(ctr + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return 0;
    }
    atomicOr(ctr + 1, 1ull);
    return 0;
}

// the key's slot, KSET_EMPTY when the set does not hold it
__device__ __forceinline__ uint64_t ks_find(const uint64_t* __restrict__ table, uint64_t slots, uint64_t key) {
    uint64_t s = ks_home(key, slots);
    for (uint64_t probe = 0; probe < slots; ++probe) {
        const uint64_t cur = table[s];
        if (cur == key) return s;
        if (cur == KSET_EMPTY) return KSET_EMPTY;
        if (++s == slots) s = 0;
    }
    return KSET_EMPTY;
}
// (the same probe as a yes or no, kept as it is: the read-only kernels compile to other code when they go through ks_find)
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

// ks_contains against R_t = { keys whose count byte is at least t } (hypo --qv-min-count): the same walk, and a hit loads the slot's byte
// of the count plane (byte s of `counts` belongs to slot s; a key's byte is at least 1 from its first window on).  One more
// dependent load per hit, none per miss.  Bounds: s < slots, and the plane has ks_plane_words(slots) * 4 >= slots bytes.
__device__ __forceinline__ bool ks_contains_min(const uint64_t* __restrict__ table, uint64_t slots, const uint8_t* __restrict__ counts, uint64_t key,
                                                uint32_t t) {
    uint64_t s = ks_home(key, slots);
    for (uint64_t probe = 0; probe < slots; ++probe) {
        const uint64_t cur = table[s];
        if (cur == key) return counts[s] >= t;
        if (cur == KSET_EMPTY) return false;
        if (++s == slots) s = 0;
    }
    return false;
}

// the last sequence that starts at or before `pos` < n = off[n_seqs] (empty ones before it are skipped): an upper-bound search
__device__ __forceinline__ uint32_t ks_seq_of(const uint64_t* __restrict__ off, uint32_t n_seqs, uint64_t pos) {
    uint32_t lo = 1, hi = n_seqs;                               // first index in [1, n_seqs] with off[index] > pos
    while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (off[mid] > pos) hi = mid; else lo = mid + 1; }
    return lo - 1;
}

__device__ __forceinline__ void ks_wave_add(unsigned long long* dst, uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(dst, (unsigned long long)v);
}

// Four slots' bytes share a 32-bit word of a plane (the count bytes of the reads, the copy bytes of a text): byte `slot` of `plane`
// goes up by one and stops at 255, with a compare-and-swap on the word that holds it.  The lane loads first (relaxed, agent scope,
// as ks_insert does): a byte that reads 255 stays 255 for good, so a hot key (poly-A, a read repeated a million times) costs no
// atomic after its 255th occurrence.  Otherwise saturation is decided on the value the atomic returns: a swap that loses hands back
// the word as it is now, the byte is looked at again in that word, and the sum is only ever swapped in against the word it was
// made from, so no byte wraps and no neighbour is touched.  Lock-free: a swap fails only because another lane's went through, and a
// word takes at most 4 * 255 increments before every byte of it is full, so the loop ends after at most 1021 rounds whatever the
// input is.  Bounds: slot < slots, and a plane has ks_plane_words(slots) words.
__device__ __forceinline__ void ks_byte_inc(uint32_t* plane, uint64_t slot) {
    uint32_t* w = plane + (slot >> 2);
    const uint32_t sh = 8u * (uint32_t)(slot & 3);
    uint32_t cur = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (((cur >> sh) & 0xffu) != 0xffu) {
        const uint32_t prev = atomicCAS(w, cur, cur + (1u << sh));
        if (prev == cur) return;
        cur = prev;
    }
}

// The body of kset_insert_kernel, and with COUNT of kset_insert_count_kernel: the probe hands back the key's slot and the slot's
// count byte goes up by one for every window.  A lane owns the windows that START in its stretch, so the windows of a launch are
// disjoint and each is counted once; the pieces of a call overlap by exactly k - 1 bytes (hypo_gpu_kset_add), so no window is in two.
template <bool COUNT>
__device__ __forceinline__ void ks_insert_body(const uint8_t* __restrict__ bytes, uint64_t n, uint32_t k, uint64_t* table, uint64_t slots,
                                               unsigned long long* ctr, uint32_t* counts) {
    __shared__ __attribute__((aligned(16))) uint8_t sb[KR_BLOCK_BYTES + KR_HALO];
    kmer_stage(sb, bytes, (uint64_t)blockIdx.x * KR_BLOCK_BYTES, n);
    const int s0 = threadIdx.x * KR_STRETCH;
    const int last = s0 + KR_STRETCH + (int)k - 1;              // exclusive end of the bytes this lane reads
    KmerRoll roll(k);
    uint32_t n_new = 0;
    for (int p = s0; p < last; ++p) {
        if (!roll.push(sb[p])) continue;                        // (a window that ends at p starts at p - k + 1 >= s0)
        if (COUNT) {
            uint64_t at;
            n_new += ks_insert<true>(table, slots, roll.canon(), ctr, &at);
            if (at != KSET_EMPTY) ks_byte_inc(counts, at);
        } else {
            n_new += ks_insert(table, slots, roll.canon(), ctr);
        }
    }
    ks_wave_add(ctr, n_new);
}

__global__ void __launch_bounds__(KS_THREADS) kset_insert_kernel(const uint8_t* __restrict__ bytes, uint64_t n, uint32_t k,
                                                                  uint64_t* table, uint64_t slots, unsigned long long* ctr) {
    ks_insert_body<false>(bytes, n, k, table, slots, ctr, nullptr);
}

__global__ void __launch_bounds__(KS_THREADS) kset_insert_count_kernel(const uint8_t* __restrict__ bytes, uint64_t n, uint32_t k,
                                                                        uint64_t* table, uint64_t slots, unsigned long long* ctr,
                                                                        uint32_t* counts) {
    ks_insert_body<true>(bytes, n, k, table, slots, ctr, counts);
}

// COUNT: the key's count byte moves with it.  Every key of the old table is there once, so a slot of the new table is claimed by one
// lane, which stores the slot's byte (the fresh plane is zero, and the copy bytes are still all zero when a table can grow).
template <bool COUNT>
__device__ __forceinline__ void ks_rehash_body(const uint64_t* __restrict__ old_table, uint64_t old_slots, uint64_t* table, uint64_t slots,
                                               unsigned long long* ctr, const uint8_t* __restrict__ old_counts, uint8_t* counts) {
    uint32_t n_new = 0;
    const uint64_t stride = (uint64_t)gridDim.x * KS_THREADS;
    for (uint64_t i = (uint64_t)blockIdx.x * KS_THREADS + threadIdx.x; i < old_slots; i += stride) {
        const uint64_t key = old_table[i];
        if (key == KSET_EMPTY) continue;
        if (COUNT) {
            uint64_t at;
            n_new += ks_insert<true>(table, slots, key, ctr, &at);
            if (at != KSET_EMPTY) counts[at] = old_counts[i];
        } else {
            n_new += ks_insert(table, slots, key, ctr);
        }
    }
    ks_wave_add(ctr, n_new);
}

__global__ void __launch_bounds__(KS_THREADS) kset_rehash_kernel(const uint64_t* __restrict__ old_table, uint64_t old_slots,
                                                                  uint64_t* table, uint64_t slots, unsigned long long* ctr) {
    ks_rehash_body<false>(old_table, old_slots, table, slots, ctr, nullptr, nullptr);
}

__global__ void __launch_bounds__(KS_THREADS) kset_rehash_count_kernel(const uint64_t* __restrict__ old_table, uint64_t old_slots,
                                                                        uint64_t* table, uint64_t slots, unsigned long long* ctr,
                                                                        const uint8_t* __restrict__ old_counts, uint8_t* counts) {
    ks_rehash_body<true>(old_table, old_slots, table, slots, ctr, old_counts, counts);
}

// The body of kset_query_kernel; as KS_TRACK of kset_track_flags_kernel (further down), which also keeps what the lane knows
// anyway: the missing bits of the 32 windows that start in its stretch, and which of its 32 bytes begin a sequence; as KS_MARK of
// kset_mark_kernel (hypo --qv-spectra): the probe hands back the slot, a window whose key is in the set adds one to that slot's byte
// of `marks` (the copy bytes of one text), and the windows and misses of all sequences go to total[0] / missing[0], per wave;
// as KS_QUERY_MIN / KS_TRACK_MIN (hypo --qv-min-count) of kset_query_min_kernel / kset_track_flags_min_kernel: KS_QUERY / KS_TRACK
// with ks_contains_min as the probe, so a window whose key the reads have fewer than min_count times is missing.
enum { KS_QUERY = 0, KS_TRACK = 1, KS_MARK = 2, KS_QUERY_MIN = 3, KS_TRACK_MIN = 4 };
template <int MODE>
__device__ __forceinline__ void ks_query_body(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ off, uint32_t n_seqs, uint64_t n,
                                              uint32_t k, const uint64_t* __restrict__ table, uint64_t slots, unsigned long long* total,
                                              unsigned long long* missing, const uint8_t* __restrict__ want, uint32_t* __restrict__ miss_bits,
                                              uint32_t* __restrict__ begin_bits, uint32_t* marks, const uint8_t* __restrict__ counts = nullptr,
                                              uint32_t min_count = 1) {
    constexpr bool TRACK = MODE == KS_TRACK || MODE == KS_TRACK_MIN, MARK = MODE == KS_MARK, MIN = MODE == KS_QUERY_MIN || MODE == KS_TRACK_MIN;
    __shared__ __attribute__((aligned(16))) uint8_t sb[KR_BLOCK_BYTES + KR_HALO];
    const uint64_t b0 = (uint64_t)blockIdx.x * KR_BLOCK_BYTES;
    kmer_stage(sb, bytes, b0, n);
    const int s0 = threadIdx.x * KR_STRETCH;
    const int last = s0 + KR_STRETCH + (int)k - 1;
    uint32_t seq = 0;
    uint64_t seq_end = 0;
    unsigned long long tot = 0, mis = 0;
    uint32_t mbits = 0, bbits = 0;                              // TRACK: bit j speaks of position b0 + s0 + j
    if (b0 + (uint64_t)s0 < n) {
        const uint64_t g0 = b0 + (uint64_t)s0;
        seq = ks_seq_of(off, n_seqs, g0);                       // the sequence that holds the lane's first byte
        seq_end = off[seq + 1];
        bool wanted = true;                                     // TRACK: the sequence in hand gets intervals
        if (TRACK) { bbits = off[seq] == g0; wanted = !want || want[seq]; }
        KmerRoll roll(k);
        for (int p = s0; p < last; ++p) {
            const uint64_t g = b0 + (uint64_t)p;
            if (g >= n) break;
            if (g == seq_end) {                                  // the next sequence starts here (g < n: there is one that holds g)
                if (!MARK) {
                    if (tot) { atomicAdd(total + seq, tot); if (mis) atomicAdd(missing + seq, mis); }
                    tot = mis = 0;
                }
                roll.reset();
                do { ++seq; seq_end = off[seq + 1]; } while (seq_end == g);
                if (TRACK) { if (p < s0 + KR_STRETCH) bbits |= 1u << (p - s0); wanted = !want || want[seq]; }
            }
            if (!roll.push(sb[p])) continue;
            ++tot;
            if (MARK) {
                const uint64_t at = ks_find(table, slots, roll.canon());
                if (at != KSET_EMPTY) ks_byte_inc(marks, at); else ++mis;
                continue;
            }
            if (MIN ? !ks_contains_min(table, slots, counts, roll.canon(), min_count) : !ks_contains(table, slots, roll.canon())) {
                ++mis;
                if (TRACK && wanted) mbits |= 1u << (p - ((int)k - 1) - s0);   // the window's start: s0 <= p - k + 1 < s0 + KR_STRETCH
            }
        }
    }
    if (TRACK) {                                                // every lane of the grid stores its two words, zero beyond n
        const uint64_t w = (uint64_t)blockIdx.x * KS_THREADS + threadIdx.x;
        miss_bits[w] = mbits; begin_bits[w] = bbits;
    }
    // per wave: the lanes that ended in the sequence of the wave's first lane are summed and added once, the others add their own
    // (MARK: one sum for all sequences, so every lane is with the first)
    const uint32_t lead = MARK ? 0u : __shfl(seq, 0);
    const bool same = MARK || seq == lead;
    unsigned long long t = same ? tot : 0, m = same ? mis : 0;
    for (int o = 32; o > 0; o >>= 1) { t += __shfl_xor(t, o); m += __shfl_xor(m, o); }
    if ((threadIdx.x & 63) == 0 && t) { atomicAdd(total + lead, t); if (m) atomicAdd(missing + lead, m); }
    if (!same && tot) { atomicAdd(total + seq, tot); if (mis) atomicAdd(missing + seq, mis); }
}

__global__ void __launch_bounds__(KS_THREADS) kset_query_kernel(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ off,
                                                                 uint32_t n_seqs, uint64_t n, uint32_t k, const uint64_t* __restrict__ table,
                                                                 uint64_t slots, unsigned long long* total, unsigned long long* missing) {
    ks_query_body<KS_QUERY>(bytes, off, n_seqs, n, k, table, slots, total, missing, nullptr, nullptr, nullptr, nullptr);
}

// ---- read counts and copy numbers (hypo --qv-spectra; DESIGN.md "k-mer spectra") ------------------------------------------------------
// Beside the table lie 1 + n_texts planes of one byte per slot, ks_plane_words(slots) 32-bit words each: plane 0 counts the
// windows of the reads per key (kset_insert_count_kernel, moved by kset_rehash_count_kernel), plane 1 + t the windows of text t
// (kset_mark_kernel).  Both stop at 255 (ks_byte_inc).  A key is in the table from its first window on, and that window counts:
// a slot's count byte is 0 exactly when the slot is free, so kset_spectrum_kernel reads the two planes and never the keys.
//   * kset_spectrum_kernel: grid-stride over the words of the count plane; every workgroup keeps the 256 x 5 bins (count, copy
//     number capped at 4) as 32-bit counters in LDS and adds the bins it used to hist[] with 64-bit adds.  Integers only: the
//     result does not depend on the order.  A workgroup sees at most 4 * ceil(words / lanes of the grid) slots, below 2^32 for any
//     table that fits a device.  Bounds: words below n_words of both planes, bins below KSET_HIST_BINS (a byte times 5 + at most 4).
__global__ void __launch_bounds__(KS_THREADS) kset_mark_kernel(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ off, uint32_t n_seqs,
                                                                uint64_t n, uint32_t k, const uint64_t* __restrict__ table, uint64_t slots,
                                                                uint32_t* marks, unsigned long long* sums) {
    ks_query_body<KS_MARK>(bytes, off, n_seqs, n, k, table, slots, sums, sums + 1, nullptr, nullptr, nullptr, marks);
}

__global__ void __launch_bounds__(KS_THREADS) kset_spectrum_kernel(const uint32_t* __restrict__ counts, const uint32_t* __restrict__ copies,
                                                                    uint64_t n_words, unsigned long long* hist) {
    __shared__ uint32_t bins[KSET_HIST_BINS];
    for (uint32_t b = threadIdx.x; b < KSET_HIST_BINS; b += KS_THREADS) bins[b] = 0;
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * KS_THREADS;
    for (uint64_t w = (uint64_t)blockIdx.x * KS_THREADS + threadIdx.x; w < n_words; w += stride) {
        const uint32_t c4 = counts[w];
        if (!c4) continue;                                      // four free slots
        const uint32_t m4 = copies[w];
        for (uint32_t j = 0; j < 32; j += 8) {
            const uint32_t c = (c4 >> j) & 0xffu, m = (m4 >> j) & 0xffu;
            if (c) atomicAdd(&bins[c * KSET_HIST_COLS + (m < KSET_HIST_COLS - 1 ? m : KSET_HIST_COLS - 1)], 1u);
        }
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < KSET_HIST_BINS; b += KS_THREADS)
        if (bins[b]) atomicAdd(hist + b, (unsigned long long)bins[b]);
}

// ---- where the missing windows are (hypo --qv-bed; DESIGN.md "k-mer QV track") -------------------------------------------------------
// Flag word w speaks of positions [32 w, 32 w + 32) of the call's bytes: miss_bits has a bit per missing window START (of a sequence
// that wants intervals), begin_bits a bit per first byte of a sequence.  kset_track_flags_kernel is the query kernel and stores the
// two words of every lane of its grid, which has one workgroup more than the bytes need when n is a multiple of KR_BLOCK_BYTES:
// position n, where the last interval may END, has a word too.  Everything after it is arithmetic on those words:
//   * a base i is covered when a missing window starts in [i - k + 1, i].  Windows never cross a sequence end, so neither does the
//     cover of one, and k <= 31 < 32: the covered bits of word w are an OR of k shifts of the 64 bits (miss[w] : miss[w - 1]),
//     done with log2 k doubling steps.
//   * an interval STARTS at a covered i whose predecessor is not covered or which begins a sequence, and ENDS (exclusive) at an i whose
//     predecessor is covered and which is not covered or begins a sequence.  Intervals are disjoint and ascending, so the j-th start
//     and the j-th end of the call belong together, and the interval's missing windows are the missing bits in front of its end less
//     those in front of its start: no lane walks an interval.
//   * kset_track_count_kernel: per workgroup the number of starts, ends and missing bits of its 256 words, one plain store.
//   * kset_track_scan_kernel: ONE workgroup turns those into exclusive prefixes, a tile of KS_SCAN_THREADS sums per pass, and leaves
//     the call's totals behind the last one.
//   * kset_track_emit_kernel: the same marks again (cheaper than keeping them), a workgroup-wide exclusive scan, and every start /
//     end bit writes its position and the missing bits in front of it into the slot of its rank.
//   * kset_track_offsets_kernel / kset_track_finish_kernel: iv_off[s] = the intervals that start before off[s] (a binary search per
//     sequence); then per interval the two counts become one and the positions become relative to the interval's sequence.
// No kernel waits for another workgroup, none uses an atomic, and every value is a function of the flag words alone.
// Bounds: flag words are indexed below n_words = gridDim.x * KS_THREADS of the flags kernel (the count and emit kernels are launched
// with the same grid); sums below n_blocks, prefixes below 3 (n_blocks + 1); interval slots below `cap` (checked per store: the
// caller sizes the arrays from the totals of the scan); iv_off below n_seqs + 1.  Loops: doubling steps <= 5, set bits of a word
// <= 32, scan passes = ceil(n_blocks / KS_SCAN_THREADS), binary searches <= 64 steps.
constexpr int KS_SCAN_THREADS = KS_THREADS;

__global__ void __launch_bounds__(KS_THREADS) kset_track_flags_kernel(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ off,
                                                                       uint32_t n_seqs, uint64_t n, uint32_t k, const uint64_t* __restrict__ table,
                                                                       uint64_t slots, unsigned long long* total, unsigned long long* missing,
                                                                       const uint8_t* __restrict__ want, uint32_t* __restrict__ miss_bits,
                                                                       uint32_t* __restrict__ begin_bits) {
    ks_query_body<KS_TRACK>(bytes, off, n_seqs, n, k, table, slots, total, missing, want, miss_bits, begin_bits, nullptr);
}

// ---- a least count (hypo --qv-min-count; DESIGN.md "k-mer min count") ---------------------------------------------------------------
// R_t = the keys the reads have at least t times, t = 2..255 (t = 1 is the set itself, and the host then launches the kernels
// above).  A set that counts answers its four queries against R_t with the kernels below: the bodies above with ks_contains_min
// as the probe, `counts` = plane 0 as bytes, `t` wave-uniform.  Everything behind the flag words of the track (count, scan, emit,
// offsets, finish) and kset_variants_reduce_kernel take their input as it is.  Bounds: those of the kernels they restate, and the
// count byte of a slot < slots.
__global__ void __launch_bounds__(KS_THREADS) kset_query_min_kernel(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ off,
                                                                     uint32_t n_seqs, uint64_t n, uint32_t k, const uint64_t* __restrict__ table,
                                                                     uint64_t slots, unsigned long long* total, unsigned long long* missing,
                                                                     const uint8_t* __restrict__ counts, uint32_t t) {
    ks_query_body<KS_QUERY_MIN>(bytes, off, n_seqs, n, k, table, slots, total, missing, nullptr, nullptr, nullptr, nullptr, counts, t);
}

__global__ void __launch_bounds__(KS_THREADS) kset_track_flags_min_kernel(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ off,
                                                                           uint32_t n_seqs, uint64_t n, uint32_t k, const uint64_t* __restrict__ table,
                                                                           uint64_t slots, unsigned long long* total, unsigned long long* missing,
                                                                           const uint8_t* __restrict__ want, uint32_t* __restrict__ miss_bits,
                                                                           uint32_t* __restrict__ begin_bits, const uint8_t* __restrict__ counts, uint32_t t) {
    ks_query_body<KS_TRACK_MIN>(bytes, off, n_seqs, n, k, table, slots, total, missing, want, miss_bits, begin_bits, nullptr, counts, t);
}

// the start and end bits of a word from the missing bits of the word before it and its own, and its begin bits
__device__ __forceinline__ void ks_track_marks(uint32_t m_prev, uint32_t m_cur, uint32_t begins, uint32_t k, uint32_t& starts, uint32_t& ends) {
    uint64_t r = ((uint64_t)m_cur << 32) | m_prev;              // bit 32 + j: position j of the word
    uint32_t width = 1;                                         // r holds the OR of its shifts by 0 .. width - 1
    for (; 2 * width <= k; width *= 2) r |= r << width;
    r |= r << (k - width);                                      // (k - width < width: no gap)
    const uint32_t cov = (uint32_t)(r >> 32), cov_before = (uint32_t)(r >> 31);
    starts = cov & (~cov_before | begins);
    ends = cov_before & (~cov | begins);
}

// A workgroup has 8192 positions, so its three counts fit 16 bits each with room to spare and travel as one 64-bit word:
// starts | ends << 16 | missing bits << 32.
__device__ __forceinline__ uint64_t ks_track_word_counts(const uint32_t* __restrict__ miss_bits, const uint32_t* __restrict__ begin_bits, uint64_t w,
                                                         uint32_t k, uint32_t& m_cur, uint32_t& starts, uint32_t& ends) {
    const uint32_t m_prev = w ? miss_bits[w - 1] : 0u;
    m_cur = miss_bits[w];
    ks_track_marks(m_prev, m_cur, begin_bits[w], k, starts, ends);
    return (uint64_t)__popc(starts) | ((uint64_t)__popc(ends) << 16) | ((uint64_t)__popc(m_cur) << 32);
}

__device__ __forceinline__ uint64_t ks_wave_inclusive(uint64_t v) {
    const uint32_t lane = threadIdx.x & 63;
    for (int o = 1; o < 64; o <<= 1) { const uint64_t u = __shfl_up(v, o); if (lane >= (uint32_t)o) v += u; }
    return v;
}

__global__ void __launch_bounds__(KS_THREADS) kset_track_count_kernel(const uint32_t* __restrict__ miss_bits, const uint32_t* __restrict__ begin_bits,
                                                                       uint32_t k, uint64_t* __restrict__ sums) {
    __shared__ uint64_t part[KS_THREADS / 64];
    uint32_t m_cur, starts, ends;
    uint64_t v = ks_track_word_counts(miss_bits, begin_bits, (uint64_t)blockIdx.x * KS_THREADS + threadIdx.x, k, m_cur, starts, ends);
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) sums[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

// pre[3 b + f]: field f (0 starts, 1 ends, 2 missing bits) summed over the workgroups before b; pre[3 n_blocks + f]: the call's totals
__global__ void __launch_bounds__(KS_SCAN_THREADS) kset_track_scan_kernel(const uint64_t* __restrict__ sums, uint32_t n_blocks, uint64_t* __restrict__ pre) {
    constexpr int WAVES = KS_SCAN_THREADS / 64;
    __shared__ uint64_t part[WAVES][3];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint64_t carry[3] = {0, 0, 0};
    for (uint32_t base = 0; base < n_blocks; base += KS_SCAN_THREADS) {
        const uint32_t i = base + threadIdx.x;
        const uint64_t packed = i < n_blocks ? sums[i] : 0;
        const uint64_t v[3] = {packed & 0xffffu, (packed >> 16) & 0xffffu, packed >> 32};
        uint64_t inc[3];
        for (int f = 0; f < 3; ++f) inc[f] = ks_wave_inclusive(v[f]);
        if (lane == 63) for (int f = 0; f < 3; ++f) part[wave][f] = inc[f];
        __syncthreads();
        for (int f = 0; f < 3; ++f) {
            uint64_t before = carry[f], all = 0;
            for (int x = 0; x < WAVES; ++x) { const uint64_t t = part[x][f]; if ((uint32_t)x < wave) before += t; all += t; }
            if (i < n_blocks) pre[3 * (uint64_t)i + f] = before + inc[f] - v[f];
            carry[f] += all;
        }
        __syncthreads();                                        // (part is written again in the next pass)
    }
    if (threadIdx.x == 0) for (int f = 0; f < 3; ++f) pre[3 * (uint64_t)n_blocks + f] = carry[f];
}

__global__ void __launch_bounds__(KS_THREADS) kset_track_emit_kernel(const uint32_t* __restrict__ miss_bits, const uint32_t* __restrict__ begin_bits,
                                                                      uint32_t k, const uint64_t* __restrict__ pre, uint64_t cap,
                                                                      uint64_t* __restrict__ iv_start, uint64_t* __restrict__ iv_end,
                                                                      uint64_t* __restrict__ cnt_lo, uint64_t* __restrict__ cnt_hi) {
    __shared__ uint64_t part[KS_THREADS / 64];
    const uint64_t w = (uint64_t)blockIdx.x * KS_THREADS + threadIdx.x;
    uint32_t m_cur, starts, ends;
    const uint64_t v = ks_track_word_counts(miss_bits, begin_bits, w, k, m_cur, starts, ends);
    const uint64_t inc = ks_wave_inclusive(v);
    if ((threadIdx.x & 63) == 63) part[threadIdx.x >> 6] = inc;
    __syncthreads();
    uint64_t ex = inc - v;                                      // what the workgroup's lanes before this one counted
    for (uint32_t x = 0; x < (threadIdx.x >> 6); ++x) ex += part[x];
    uint64_t rank_s = pre[3 * (uint64_t)blockIdx.x] + (ex & 0xffffu), rank_e = pre[3 * (uint64_t)blockIdx.x + 1] + ((ex >> 16) & 0xffffu);
    const uint64_t m_before = pre[3 * (uint64_t)blockIdx.x + 2] + (ex >> 32);
    while (starts) {
        const uint32_t j = (uint32_t)__ffs(starts) - 1;
        starts &= starts - 1;
        if (rank_s < cap) { iv_start[rank_s] = w * 32 + j; cnt_lo[rank_s] = m_before + __popc(m_cur & ((1u << j) - 1u)); }
        ++rank_s;
    }
    while (ends) {
        const uint32_t j = (uint32_t)__ffs(ends) - 1;
        ends &= ends - 1;
        if (rank_e < cap) { iv_end[rank_e] = w * 32 + j; cnt_hi[rank_e] = m_before + __popc(m_cur & ((1u << j) - 1u)); }
        ++rank_e;
    }
}

// iv_off[s] = the first interval that starts at or after off[s], s = 0 .. n_seqs (iv_start ascends)
__global__ void __launch_bounds__(KS_THREADS) kset_track_offsets_kernel(const uint64_t* __restrict__ off, uint32_t n_seqs, const uint64_t* __restrict__ iv_start,
                                                                         uint64_t n_iv, uint64_t* __restrict__ iv_off) {
    const uint64_t s = (uint64_t)blockIdx.x * KS_THREADS + threadIdx.x;
    if (s > n_seqs) return;
    const uint64_t at = off[s];
    uint64_t lo = 0, hi = n_iv;
    while (lo < hi) { const uint64_t mid = lo + (hi - lo) / 2; if (iv_start[mid] >= at) hi = mid; else lo = mid + 1; }
    iv_off[s] = lo;
}

// per interval: cnt_hi becomes its missing windows, its positions become relative to the sequence that holds its start
__global__ void __launch_bounds__(KS_THREADS) kset_track_finish_kernel(const uint64_t* __restrict__ off, uint32_t n_seqs, uint64_t n_iv,
                                                                        uint64_t* __restrict__ iv_start, uint64_t* __restrict__ iv_end,
                                                                        const uint64_t* __restrict__ cnt_lo, uint64_t* __restrict__ cnt_hi) {
    const uint64_t j = (uint64_t)blockIdx.x * KS_THREADS + threadIdx.x;
    if (j >= n_iv) return;
    const uint64_t at = iv_start[j];
    const uint64_t base = off[ks_seq_of(off, n_seqs, at)];      // (off[n_seqs] = n > at)
    iv_start[j] = at - base;
    iv_end[j] -= base;
    cnt_hi[j] -= cnt_lo[j];
}

uint32_t kset_track_blocks(uint64_t n) { return (uint32_t)(n / KR_BLOCK_BYTES + 1); }

hipError_t kset_track_count_run(const KsetView& set, const uint8_t* bytes, const uint64_t* off, uint32_t n_seqs, uint64_t n, unsigned long long* total,
                                unsigned long long* missing, const uint8_t* want, uint32_t* miss_bits, uint32_t* begin_bits, uint64_t* sums, uint64_t* pre,
                                hipStream_t st) {
    const uint32_t blocks = kset_track_blocks(n);
    if (set.min_count > 1)
        kset_track_flags_min_kernel<<<dim3(blocks), dim3(KS_THREADS), 0, st>>>(bytes, off, n_seqs, n, set.k, set.table, set.slots, total, missing, want, miss_bits,
                                                                               begin_bits, (const uint8_t*)set.planes, set.min_count);
    else
        kset_track_flags_kernel<<<dim3(blocks), dim3(KS_THREADS), 0, st>>>(bytes, off, n_seqs, n, set.k, set.table, set.slots, total, missing, want, miss_bits, begin_bits);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    kset_track_count_kernel<<<dim3(blocks), dim3(KS_THREADS), 0, st>>>(miss_bits, begin_bits, set.k, sums);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    kset_track_scan_kernel<<<dim3(1), dim3(KS_SCAN_THREADS), 0, st>>>(sums, blocks, pre);
    return hipGetLastError();
}

hipError_t kset_track_emit_run(const uint64_t* off, uint32_t n_seqs, uint64_t n, uint32_t k, const uint32_t* miss_bits, const uint32_t* begin_bits,
                               const uint64_t* pre, uint64_t n_iv, uint64_t* iv_off, uint64_t* iv_start, uint64_t* iv_end, uint64_t* cnt_lo,
                               uint64_t* cnt_hi, hipStream_t st) {
    hipError_t e = hipSuccess;
    if (n_iv) {
        kset_track_emit_kernel<<<dim3(kset_track_blocks(n)), dim3(KS_THREADS), 0, st>>>(miss_bits, begin_bits, k, pre, n_iv, iv_start, iv_end, cnt_lo, cnt_hi);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    kset_track_offsets_kernel<<<dim3(n_seqs / KS_THREADS + 1), dim3(KS_THREADS), 0, st>>>(off, n_seqs, iv_start, n_iv, iv_off);
    if ((e = hipGetLastError()) != hipSuccess || !n_iv) return e;
    kset_track_finish_kernel<<<dim3((uint32_t)((n_iv + KS_THREADS - 1) / KS_THREADS)), dim3(KS_THREADS), 0, st>>>(off, n_seqs, n_iv, iv_start, iv_end, cnt_lo, cnt_hi);
    return hipGetLastError();
}

// ---- many short spans (hypo --kmer-guard; DESIGN.md "k-mer guard") -------------------------------------------------------------------
// A group of G lanes (a half-wave or a wave) owns one item, a piece of a span with at most KSET_SPAN_PIECE windows (the host cuts
// longer spans, so one long span among short ones is spread over many groups).  The group walks its item in passes of G windows.
// In a pass every lane loads ONE byte, the next G bytes of the item, and three ballots turn the group's bytes into bit masks: the
// low bit of the base code, its high bit, and "not a base".  The masks of the pass before are carried (a window needs k - 1 <= G
// bytes beyond its first), so every byte is loaded once.  Lane l's window is bits [l, l + k) of the two masks in hand: the forward
// code is their bit-reversed interleave (MSB-first), the reverse complement the interleave of their complements.  No LDS, no
// per-lane loop over bytes.  Hits and misses are counted with two more ballots, so the sums are wave-uniform and the group's first
// lane stores them; no atomics, and the output is a pure function of the input.
// All of that is ks_group_scan; a kernel reads its item's descriptor and says where byte x of the item is.
__device__ __forceinline__ uint64_t ks_spread(uint64_t x) {     // bit j of the low 32 bits to bit 2j
    x &= 0xffffffffull;
    x = (x | (x << 16)) & 0x0000ffff0000ffffull;
    x = (x | (x << 8)) & 0x00ff00ff00ff00ffull;
    x = (x | (x << 4)) & 0x0f0f0f0f0f0f0f0full;
    x = (x | (x << 2)) & 0x3333333333333333ull;
    x = (x | (x << 1)) & 0x5555555555555555ull;
    return x;
}

template <int G> __device__ __forceinline__ uint64_t ks_group_part(uint64_t wave_mask, uint32_t half) {
    return G == 64 ? wave_mask : (wave_mask >> (32 * half)) & 0xffffffffull;
}
// bits [l, l + 32) of the 2G bits (hi : lo)
template <int G> __device__ __forceinline__ uint32_t ks_window_bits(uint64_t lo, uint64_t hi, uint32_t l) {
    if (G == 32) return (uint32_t)(((hi << 32) | lo) >> l);
    return (uint32_t)(l ? (lo >> l) | (hi << (64 - l)) : lo);
}

// The item of the calling lane's group goes through the set: `fetch(x)` is byte x < len of the item, out[item] = (windows, misses).
// MIN (hypo --qv-min-count): the probe is ks_contains_min with `counts` and `t`.
template <int G, bool MIN, class Fetch>
__device__ __forceinline__ void ks_group_scan(Fetch fetch, bool have, uint32_t len, uint32_t k, const uint64_t* __restrict__ table,
                                              uint64_t slots, uint2* __restrict__ out, uint64_t item, const uint8_t* __restrict__ counts = nullptr,
                                              uint32_t t = 1) {
    static_assert(G == 32 || G == 64, "a half-wave or a wave");
    const uint32_t lane = threadIdx.x & 63, l = lane & (G - 1), half = G == 64 ? 0 : lane >> 5;
    const uint32_t n_win = len >= k ? len - k + 1 : 0;
    const uint32_t kmask = (uint32_t)((1ull << k) - 1);
    auto load_masks = [&](uint32_t at, uint64_t& b0, uint64_t& b1, uint64_t& bad) {   // bytes [at, at + G) of the item (wave-uniform call)
        const uint32_t x = at + l;
        const uint32_t c = x < len ? base_code(fetch(x)) : 4u;
        b0 = ks_group_part<G>(__ballot(c & 1u), half);
        b1 = ks_group_part<G>(__ballot(c & 2u), half);
        bad = ks_group_part<G>(__ballot(c > 3u), half);
    };
    uint64_t c0, c1, cb, n0, n1, nb;                           // the masks of the pass's G bytes, and of the G bytes after them
    load_masks(0, c0, c1, cb);
    uint32_t tot = 0, mis = 0;
    // (both halves of a wave stay in the loop until the longer item is done; variant lengths differ per mask)
    for (uint32_t base = 0; __any(base < n_win); base += G) {
        load_masks(base + G, n0, n1, nb);
        const bool in = base + l < n_win;
        const bool ok = in && (ks_window_bits<G>(cb, nb, l) & kmask) == 0;
        bool miss = false;
        if (ok) {
            const uint32_t h0 = ks_window_bits<G>(c0, n0, l) & kmask, h1 = ks_window_bits<G>(c1, n1, l) & kmask;
            const uint64_t fwd = (ks_spread(__brev(h1) >> (32 - k)) << 1) | ks_spread(__brev(h0) >> (32 - k));
            const uint64_t rc = (ks_spread(~h1 & kmask) << 1) | ks_spread(~h0 & kmask);
            const uint64_t key = fwd < rc ? fwd : rc;
            miss = MIN ? !ks_contains_min(table, slots, counts, key, t) : !ks_contains(table, slots, key);
        }
        tot += (uint32_t)__popcll(ks_group_part<G>(__ballot(ok), half));
        mis += (uint32_t)__popcll(ks_group_part<G>(__ballot(miss), half));
        c0 = n0; c1 = n1; cb = nb;
    }
    if (have && l == 0) out[item] = make_uint2(tot, mis);
}

// Bounds: a lane reads bytes[lo + x] for x < len only (lo + len <= n is checked by the caller); items and out are indexed below
// n_items; the probe is ks_contains (slot indices < slots, at most `slots` steps).
// (The two kernels do not share a body as the variants' and the fixes' do: through one, the compiler hands the two descriptor loads
// each other's registers, and a refactor leaves the instruction stream as it is.)
template <int G>
__global__ void __launch_bounds__(KS_THREADS) kset_spans_kernel(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ item_lo,
                                                                 const uint32_t* __restrict__ item_len, uint32_t n_items, uint32_t k,
                                                                 const uint64_t* __restrict__ table, uint64_t slots, uint2* __restrict__ out) {
    const uint64_t item = ((uint64_t)blockIdx.x * KS_THREADS + threadIdx.x) / G;
    const bool have = item < n_items;
    const uint64_t lo = have ? item_lo[item] : 0;
    ks_group_scan<G, false>([&](uint32_t x) { return (uint32_t)bytes[lo + x]; }, have, have ? item_len[item] : 0, k, table, slots, out, item);
}

// kset_spans_kernel against R_t (hypo --qv-min-count; the section "a least count" above)
template <int G>
__global__ void __launch_bounds__(KS_THREADS) kset_spans_min_kernel(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ item_lo,
                                                                     const uint32_t* __restrict__ item_len, uint32_t n_items, uint32_t k,
                                                                     const uint64_t* __restrict__ table, uint64_t slots, uint2* __restrict__ out,
                                                                     const uint8_t* __restrict__ counts, uint32_t t) {
    const uint64_t item = ((uint64_t)blockIdx.x * KS_THREADS + threadIdx.x) / G;
    const bool have = item < n_items;
    const uint64_t lo = have ? item_lo[item] : 0;
    ks_group_scan<G, true>([&](uint32_t x) { return (uint32_t)bytes[lo + x]; }, have, have ? item_len[item] : 0, k, table, slots, out, item, counts, t);
}

// The grid of a kernel whose items take a group of `group` lanes each (32 or 64): launch(G, blocks), G the group as a compile-time
// constant (decltype(G)::value), blocks the workgroups n_items need.  What it answers is hipGetLastError() after the launch.
template <class Launch> hipError_t ks_launch_groups(uint32_t n_items, int group, Launch launch) {
    const uint32_t per_block = (uint32_t)KS_THREADS / (uint32_t)group;
    const dim3 blocks((n_items + per_block - 1) / per_block);
    if (group == 32) launch(std::integral_constant<int, 32>(), blocks); else launch(std::integral_constant<int, 64>(), blocks);
    return hipGetLastError();
}

hipError_t kset_spans_run(const KsetView& set, const uint8_t* bytes, const uint64_t* item_lo, const uint32_t* item_len, uint32_t n_items, uint2* out,
                          int group, hipStream_t st) {
    if (!n_items) return hipSuccess;
    return ks_launch_groups(n_items, group, [&](auto g, dim3 blocks) {
        constexpr int G = decltype(g)::value;
        if (set.min_count > 1)
            kset_spans_min_kernel<G><<<blocks, dim3(KS_THREADS), 0, st>>>(bytes, item_lo, item_len, n_items, set.k, set.table, set.slots, out, (const uint8_t*)set.planes,
                                                                         set.min_count);
        else kset_spans_kernel<G><<<blocks, dim3(KS_THREADS), 0, st>>>(bytes, item_lo, item_len, n_items, set.k, set.table, set.slots, out);
    });
}

// ---- every subset of a site's edits (hypo --guard-records; DESIGN.md "k-mer guard by record") -------------------------------------------
// An item is a piece of ONE variant of a site: x = site, y = mask, z = the piece's first byte in the variant's text, w = its length
// (at most KSET_SPAN_PIECE windows, as the spans' pieces).  The variant's text exists nowhere: byte p of variant `mask` of a site
// is found by walking the site's (at most KSET_MAX_EDITS) edits in order with two running positions, `sp` in bytes and `vp` in the
// variant, and comes from `alts` inside an edit whose bit is set, from `bytes` otherwise.  A lane loads one such byte a pass; the
// rest is ks_group_scan, as for the spans.
// No LDS, no atomics, no scratch; item i's pair goes to out[i] and kset_variants_reduce_kernel adds the pieces up.
// Bounds: a lane asks for byte p of its item's variant only for p < z + w <= the variant's length (the caller computed both from the
// same edits), so the walk ends inside the site: bytes is read at [lo, hi) of the site, alts at [ao[e], ao[e] + al[e]) of an edit
// of the site, e in [edit_off[site], edit_off[site + 1]) — the caller checked lo <= eb_0 <= ee_0 <= ... <= hi <= n_bytes and
// ao + al <= n_alt_bytes for all of them.  items / out are indexed below n_items, sites below n_sites (the caller's items name
// sites it has), the probe is ks_contains.
__device__ __forceinline__ uint32_t ks_variant_byte(const uint8_t* __restrict__ bytes, const uint8_t* __restrict__ alts, uint64_t lo,
                                                     uint32_t e0, uint32_t e1, const uint64_t* __restrict__ eb, const uint64_t* __restrict__ ee,
                                                     const uint64_t* __restrict__ ao, const uint32_t* __restrict__ al, uint32_t mask, uint32_t p) {
    uint64_t sp = lo;                                           // bytes before sp are behind the walk
    uint32_t vp = 0;                                            // and so are the variant's bytes before vp
    for (uint32_t e = e0; e < e1; ++e) {
        const uint64_t b = eb[e], en = ee[e];
        const uint32_t keep = (uint32_t)(b - sp);               // the unchanged stretch in front of the edit
        if (p - vp < keep) return bytes[sp + (p - vp)];
        vp += keep;
        if ((mask >> (e - e0)) & 1u) {
            const uint32_t n = al[e];
            if (p - vp < n) return alts[ao[e] + (p - vp)];
            vp += n;
        } else {
            const uint32_t n = (uint32_t)(en - b);
            if (p - vp < n) return bytes[b + (p - vp)];
            vp += n;
        }
        sp = en;
    }
    return bytes[sp + (p - vp)];
}

template <int G, bool MIN>
__device__ __forceinline__ void ks_variants_body(const uint8_t* __restrict__ bytes, const uint8_t* __restrict__ alts, const uint64_t* __restrict__ site_lo,
                                                 const uint32_t* __restrict__ edit_off, const uint64_t* __restrict__ eb, const uint64_t* __restrict__ ee,
                                                 const uint64_t* __restrict__ ao, const uint32_t* __restrict__ al, const uint4* __restrict__ items,
                                                 uint32_t n_items, uint32_t k, const uint64_t* __restrict__ table, uint64_t slots, uint2* __restrict__ out,
                                                 const uint8_t* __restrict__ counts, uint32_t t) {
    const uint64_t item = ((uint64_t)blockIdx.x * KS_THREADS + threadIdx.x) / G;
    const bool have = item < n_items;
    const uint4 it = have ? items[item] : make_uint4(0, 0, 0, 0);
    const uint64_t lo = have ? site_lo[it.x] : 0;
    const uint32_t e0 = have ? edit_off[it.x] : 0, e1 = have ? edit_off[it.x + 1] : 0;
    ks_group_scan<G, MIN>([&](uint32_t x) { return ks_variant_byte(bytes, alts, lo, e0, e1, eb, ee, ao, al, it.y, it.z + x); }, have, it.w, k, table, slots, out, item,
                          counts, t);
}

template <int G>
__global__ void __launch_bounds__(KS_THREADS) kset_variants_kernel(const uint8_t* __restrict__ bytes, const uint8_t* __restrict__ alts,
                                                                    const uint64_t* __restrict__ site_lo, const uint32_t* __restrict__ edit_off,
                                                                    const uint64_t* __restrict__ eb, const uint64_t* __restrict__ ee,
                                                                    const uint64_t* __restrict__ ao, const uint32_t* __restrict__ al,
                                                                    const uint4* __restrict__ items, uint32_t n_items, uint32_t k,
                                                                    const uint64_t* __restrict__ table, uint64_t slots, uint2* __restrict__ out) {
    ks_variants_body<G, false>(bytes, alts, site_lo, edit_off, eb, ee, ao, al, items, n_items, k, table, slots, out, nullptr, 1);
}

// kset_variants_kernel against R_t (hypo --qv-min-count; the section "a least count" above)
template <int G>
__global__ void __launch_bounds__(KS_THREADS) kset_variants_min_kernel(const uint8_t* __restrict__ bytes, const uint8_t* __restrict__ alts,
                                                                        const uint64_t* __restrict__ site_lo, const uint32_t* __restrict__ edit_off,
                                                                        const uint64_t* __restrict__ eb, const uint64_t* __restrict__ ee,
                                                                        const uint64_t* __restrict__ ao, const uint32_t* __restrict__ al,
                                                                        const uint4* __restrict__ items, uint32_t n_items, uint32_t k,
                                                                        const uint64_t* __restrict__ table, uint64_t slots, uint2* __restrict__ out,
                                                                        const uint8_t* __restrict__ counts, uint32_t t) {
    ks_variants_body<G, true>(bytes, alts, site_lo, edit_off, eb, ee, ao, al, items, n_items, k, table, slots, out, counts, t);
}

// One lane per site: the pieces of every variant are added up (the site's items are in mask order, a variant's pieces next to each
// other) and the best variant is kept: fewest missing, then most edits taken, then the greatest mask — masks come in ascending
// order, so among equals the later one wins when it takes at least as many edits.  var_total / var_missing (NULL or both): every
// variant's sums at var_off[site] + mask.
// Bounds: items / res below site_item[n_sites] = n_items, best_* below n_sites, var_* below var_off[site] + 2^(edits of the site).
__global__ void __launch_bounds__(KS_THREADS) kset_variants_reduce_kernel(const uint4* __restrict__ items, const uint2* __restrict__ res,
                                                                           const uint32_t* __restrict__ site_item, const uint32_t* __restrict__ var_off,
                                                                           uint32_t n_sites, uint32_t* __restrict__ best_mask,
                                                                           unsigned long long* __restrict__ best_total, unsigned long long* __restrict__ best_missing,
                                                                           unsigned long long* __restrict__ var_total, unsigned long long* __restrict__ var_missing) {
    const uint64_t s = (uint64_t)blockIdx.x * KS_THREADS + threadIdx.x;
    if (s >= n_sites) return;
    const uint32_t i0 = site_item[s], i1 = site_item[s + 1], v0 = var_off[s];
    uint32_t bm = 0;
    unsigned long long bt = 0, bmis = 0;
    bool first = true;
    for (uint32_t i = i0; i < i1;) {
        const uint32_t m = items[i].y;
        unsigned long long t = 0, mis = 0;
        for (; i < i1 && items[i].y == m; ++i) { t += res[i].x; mis += res[i].y; }
        if (var_total) { var_total[(uint64_t)v0 + m] = t; var_missing[(uint64_t)v0 + m] = mis; }
        if (first || mis < bmis || (mis == bmis && __popc(m) >= __popc(bm))) { bm = m; bt = t; bmis = mis; first = false; }
    }
    best_mask[s] = bm; best_total[s] = bt; best_missing[s] = bmis;
}

hipError_t kset_variants_run(const KsetView& set, const KsetVariantsIn& in, const KsetVariantsOut& out, int group, hipStream_t st) {
    if (!in.n_sites || !in.n_items) return hipSuccess;
    const hipError_t e = ks_launch_groups(in.n_items, group, [&](auto g, dim3 blocks) {
        constexpr int G = decltype(g)::value;
        if (set.min_count > 1)
            kset_variants_min_kernel<G><<<blocks, dim3(KS_THREADS), 0, st>>>(in.bytes, in.alts, in.site_lo, in.edit_off, in.eb, in.ee, in.ao, in.al, in.items, in.n_items, set.k,
                                                                            set.table, set.slots, out.item_res, (const uint8_t*)set.planes, set.min_count);
        else
            kset_variants_kernel<G><<<blocks, dim3(KS_THREADS), 0, st>>>(in.bytes, in.alts, in.site_lo, in.edit_off, in.eb, in.ee, in.ao, in.al, in.items, in.n_items, set.k,
                                                                        set.table, set.slots, out.item_res);
    });
    if (e != hipSuccess) return e;
    kset_variants_reduce_kernel<<<dim3((in.n_sites + KS_THREADS - 1) / KS_THREADS), dim3(KS_THREADS), 0, st>>>(in.items, out.item_res, in.site_item, in.var_off, in.n_sites,
                                                                                                                 out.best_mask, out.best_total, out.best_missing, out.var_total,
                                                                                                                 out.var_missing);
    return hipGetLastError();
}

// ---- every one-base edit of a short region (hypo --kmer-fix; DESIGN.md "k-mer fix") -----------------------------------------------------
// An item is ONE candidate of a site: item i belongs to the site s with item_off[s] <= i < item_off[s + 1] (a binary search; a site
// with a region of w bytes has 9 w - 3 candidates) and j = i - item_off[s] names its edit by arithmetic, in the order of
// ks_fix_edit.  The candidate's text exists nowhere: byte x of it is the edit's base where x is the edit's position p, and else
// byte x of the span, one further on from p for a deletion, one back behind p for an insertion.  A lane loads one such byte a
// pass; the rest is ks_group_scan, as for the spans.  No LDS, no atomics, no scratch; item i's pair goes to out[i].
// Bounds: the caller checked lo <= c0 < c1 <= hi <= n_bytes, hi - lo <= KSET_MAX_FIX_SPAN and c1 - c0 <= KSET_MAX_FIX_REGION for
// every site.  With L = hi - lo and p in [c0 - lo, c1 - lo): a substitution has L bytes and reads lo + x, x < L; a deletion has
// L - 1 and reads lo + x + 1 <= lo + L - 1; an insertion has L + 1 and reads lo + x - 1 <= lo + L - 1 behind p, lo + x < lo + p
// in front of it.  So every read is inside [lo, hi).  A text has at most 2049 bytes: at most 2049 / G + 1 passes.  items / out
// are indexed below n_items = item_off[n_sites], sites below n_sites (the search), the probe is ks_contains.
enum { KS_FIX_NONE = 0, KS_FIX_SUB = 1, KS_FIX_DEL = 2, KS_FIX_INS = 3 };
__device__ __forceinline__ uint32_t ks_base_char(uint32_t base) { return (0x54474341u >> (8 * base)) & 0xffu; }   // 'A' 'C' 'G' 'T'
// candidate j < 9 w - 3 of a region of w bytes: its kind, its position relative to the region's first byte, its base (0..3)
__device__ __forceinline__ void ks_fix_edit(uint32_t j, uint32_t w, uint32_t& kind, uint32_t& at, uint32_t& base) {
    kind = KS_FIX_NONE; at = 0; base = 0;
    if (!j) return;
    --j;
    if (j < 4 * w) { kind = KS_FIX_SUB; at = j >> 2; base = j & 3u; return; }
    j -= 4 * w;
    if (j < w) { kind = KS_FIX_DEL; at = j; return; }
    j -= w;
    kind = KS_FIX_INS; at = 1 + (j >> 2); base = j & 3u;
}

template <int G, bool MIN>
__device__ __forceinline__ void ks_fixes_body(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ site_lo, const uint32_t* __restrict__ site_len,
                                              const uint32_t* __restrict__ site_c0, const uint32_t* __restrict__ site_w,
                                              const uint32_t* __restrict__ item_off, uint32_t n_sites, uint32_t n_items, uint32_t k,
                                              const uint64_t* __restrict__ table, uint64_t slots, uint2* __restrict__ out,
                                              const uint8_t* __restrict__ counts, uint32_t t) {
    const uint64_t item = ((uint64_t)blockIdx.x * KS_THREADS + threadIdx.x) / G;
    const bool have = item < n_items;
    uint64_t lo = 0;
    uint32_t len = 0, p = 0xffffffffu, ch = 0, kind = KS_FIX_NONE;
    if (have) {
        uint32_t a = 0, b = n_sites;                            // the last site with item_off[site] <= item (item < item_off[n_sites])
        while (b - a > 1) { const uint32_t mid = a + (b - a) / 2; if (item_off[mid] <= (uint32_t)item) a = mid; else b = mid; }
        uint32_t at, base;
        ks_fix_edit((uint32_t)item - item_off[a], site_w[a], kind, at, base);
        lo = site_lo[a];
        len = site_len[a] + (kind == KS_FIX_INS ? 1u : 0u) - (kind == KS_FIX_DEL ? 1u : 0u);
        if (kind != KS_FIX_NONE) p = site_c0[a] + at;
        ch = ks_base_char(base);
    }
    const bool put = kind == KS_FIX_SUB || kind == KS_FIX_INS;  // the byte at p is the edit's base
    const uint32_t skip = kind == KS_FIX_DEL ? 1u : kind == KS_FIX_INS ? 0xffffffffu : 0u;   // from p on: + 1, - 1 or nothing
    ks_group_scan<G, MIN>([&](uint32_t x) { return put && x == p ? ch : (uint32_t)bytes[lo + (uint32_t)(x + (x >= p ? skip : 0u))]; }, have, len, k, table, slots, out, item,
                          counts, t);
}

template <int G>
__global__ void __launch_bounds__(KS_THREADS) kset_fixes_kernel(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ site_lo,
                                                                 const uint32_t* __restrict__ site_len, const uint32_t* __restrict__ site_c0,
                                                                 const uint32_t* __restrict__ site_w, const uint32_t* __restrict__ item_off,
                                                                 uint32_t n_sites, uint32_t n_items, uint32_t k, const uint64_t* __restrict__ table,
                                                                 uint64_t slots, uint2* __restrict__ out) {
    ks_fixes_body<G, false>(bytes, site_lo, site_len, site_c0, site_w, item_off, n_sites, n_items, k, table, slots, out, nullptr, 1);
}

// kset_fixes_kernel against R_t (hypo --qv-min-count; the section "a least count" above)
template <int G>
__global__ void __launch_bounds__(KS_THREADS) kset_fixes_min_kernel(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ site_lo,
                                                                     const uint32_t* __restrict__ site_len, const uint32_t* __restrict__ site_c0,
                                                                     const uint32_t* __restrict__ site_w, const uint32_t* __restrict__ item_off,
                                                                     uint32_t n_sites, uint32_t n_items, uint32_t k, const uint64_t* __restrict__ table,
                                                                     uint64_t slots, uint2* __restrict__ out, const uint8_t* __restrict__ counts, uint32_t t) {
    ks_fixes_body<G, true>(bytes, site_lo, site_len, site_c0, site_w, item_off, n_sites, n_items, k, table, slots, out, counts, t);
}

__device__ __forceinline__ uint32_t ks_upper(uint32_t c) { return c >= 'a' && c <= 'z' ? c - 32u : c; }

// One lane per site walks the site's candidates in order.  A candidate is CANONICAL when no earlier one and not the unedited span
// spells the same text, which the region's own bytes decide: a substitution that changes the base, a deletion of the first base of
// a run (or at the region's start), an insertion that does not repeat the base in front of it (or right behind the region's
// start).  best_*: the canonical candidate with the fewest missing windows, the first among equals; zeros: the canonical
// candidates with none missing.  cand_total / cand_missing (NULL or both): every candidate's pair at item_off[site] + j.
// Bounds: res / cand_* below item_off[n_sites] = n_items, the six per-site arrays below n_sites, bytes at [c0, c1) of the site only
// (the byte in front of position q is read for q > c0 alone).
__global__ void __launch_bounds__(KS_THREADS) kset_fixes_reduce_kernel(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ site_lo,
                                                                        const uint32_t* __restrict__ site_c0, const uint32_t* __restrict__ site_w,
                                                                        const uint32_t* __restrict__ item_off, const uint2* __restrict__ res,
                                                                        uint32_t n_sites, unsigned long long* __restrict__ none_total,
                                                                        unsigned long long* __restrict__ none_missing, uint32_t* __restrict__ best_cand,
                                                                        unsigned long long* __restrict__ best_total, unsigned long long* __restrict__ best_missing,
                                                                        uint32_t* __restrict__ zeros, unsigned long long* __restrict__ cand_total,
                                                                        unsigned long long* __restrict__ cand_missing) {
    const uint64_t s = (uint64_t)blockIdx.x * KS_THREADS + threadIdx.x;
    if (s >= n_sites) return;
    const uint32_t i0 = item_off[s], w = site_w[s], n = 9 * w - 3;
    const uint8_t* reg = bytes + site_lo[s] + site_c0[s];       // the region's w bytes
    uint32_t bc = 0, nz = 0;
    unsigned long long bt = 0, bm = 0;
    bool first = true;
    for (uint32_t j = 0; j < n; ++j) {
        const uint2 r = res[i0 + j];
        if (cand_total) { cand_total[(uint64_t)i0 + j] = r.x; cand_missing[(uint64_t)i0 + j] = r.y; }
        if (!j) { none_total[s] = r.x; none_missing[s] = r.y; continue; }
        uint32_t kind, at, base;
        ks_fix_edit(j, w, kind, at, base);
        const uint32_t b = ks_base_char(base);
        bool canon;
        if (kind == KS_FIX_SUB) canon = ks_upper(reg[at]) != b;
        else if (kind == KS_FIX_DEL) canon = at == 0 || ks_upper(reg[at - 1]) != ks_upper(reg[at]);
        else canon = at == 1 || ks_upper(reg[at - 1]) != b;
        if (!canon) continue;
        if (!r.y) ++nz;
        if (first || r.y < bm) { bc = j; bt = r.x; bm = r.y; first = false; }
    }
    best_cand[s] = bc; best_total[s] = bt; best_missing[s] = bm; zeros[s] = nz;
}

hipError_t kset_fixes_run(const KsetView& set, const KsetFixesIn& in, const KsetFixesOut& out, int group, hipStream_t st) {
    if (!in.n_sites || !in.n_items) return hipSuccess;
    const hipError_t e = ks_launch_groups(in.n_items, group, [&](auto g, dim3 blocks) {
        constexpr int G = decltype(g)::value;
        if (set.min_count > 1)
            kset_fixes_min_kernel<G><<<blocks, dim3(KS_THREADS), 0, st>>>(in.bytes, in.site_lo, in.site_len, in.site_c0, in.site_w, in.item_off, in.n_sites, in.n_items, set.k,
                                                                         set.table, set.slots, out.item_res, (const uint8_t*)set.planes, set.min_count);
        else
            kset_fixes_kernel<G><<<blocks, dim3(KS_THREADS), 0, st>>>(in.bytes, in.site_lo, in.site_len, in.site_c0, in.site_w, in.item_off, in.n_sites, in.n_items, set.k,
                                                                     set.table, set.slots, out.item_res);
    });
    if (e != hipSuccess) return e;
    kset_fixes_reduce_kernel<<<dim3((in.n_sites + KS_THREADS - 1) / KS_THREADS), dim3(KS_THREADS), 0, st>>>(in.bytes, in.site_lo, in.site_c0, in.site_w, in.item_off, out.item_res,
                                                                                                              in.n_sites, out.none_total, out.none_missing, out.best_cand,
                                                                                                              out.best_total, out.best_missing, out.zeros, out.cand_total,
                                                                                                              out.cand_missing);
    return hipGetLastError();
}

// ---- walks between two anchors (hypo --kmer-bridge; DESIGN.md "k-mer bridge") ----------------------------------------------------------
// The set as a de Bruijn graph: a k-mer's children are the four k-mers that drop its first base and append one, those of them
// whose canonical code the set holds.  Site s asks for the walks from L = bytes[from, from + k) that arrive at R = bytes[to, to + k)
// after dlo .. dhi steps, a walk ending at its first arrival in that range.  The search is the depth-first one of include/hypo_gpu.h,
// children in ACGT order, every visit counted, and it answers NONE, UNIQUE, AMBIGUOUS (a second walk arrived), BUDGET (more than
// `budget` visits) or NOANCHOR (an anchor holds a byte that is no base), with the visits made and the first walk's bases.
// A group of 4 lanes owns a site, a wave 16 sites, a workgroup 64.  All four lanes carry the same state (depth, the forward and
// reverse-complement codes of the k-mer the group stands on, the counters), so every branch on it is uniform within the group.
// When the group steps onto a k-mer, lane b rolls child b as KmerRoll does, takes the canonical code and probes the table; the
// group's four bits of one wave-wide ballot are the children that exist.  The stack is one byte per depth in LDS: the children not
// tried yet in bits 0..3, the base taken last in bits 4..5.  Every lane of the group stores and loads the same bytes, so no lane
// reads what another wrote.  On a backtrack the parent's codes come back in one step from the child's: the base that fell off the
// front is base d - 1 of L + the path, which L's code or the stack still holds.  The first walk that arrives is copied from the
// stack to walk[] by the group, a byte per lane and pass, with plain stores.  No atomics, no scratch.
// The loop is wave-uniform: an iteration expands the groups that stepped onto a k-mer (the probes, one ballot), then every group
// takes its next untried child (a visit) or, with none left, steps back.  A wave runs as long as its slowest site.
// Bounds: a site makes at most `budget` <= KSET_MAX_WALK_BUDGET visits and no more steps back than visits, so the loop ends after
// at most 2 budget + 2 iterations; a probe takes at most `slots` steps; depth <= dhi <= KSET_MAX_WALK = 256, the stack is indexed
// at depth < dhi (a k-mer at depth dhi is never expanded), below KS_WALK_STACK; walk[] is written at [s * 256, s * 256 + len),
// len <= dhi; bytes are read at [from, from + k) and [to, to + k), which the caller checked to lie inside the text; status / steps
// / len are indexed below n_sites.
constexpr int KS_WALK_LANES = 4;                                // lanes per site: one per child
constexpr int KS_WALK_SITES = KS_THREADS / KS_WALK_LANES;       // sites per workgroup
constexpr int KS_WALK_STACK = 260;                              // bytes per site: 256 depths, padded so that the sites of a wave fall into different banks
enum { KS_WALK_NONE = 0, KS_WALK_UNIQUE = 1, KS_WALK_AMBIGUOUS = 2, KS_WALK_BUDGET = 3, KS_WALK_NOANCHOR = 4 };

// the forward and reverse-complement codes of bytes[at, at + k); false when one of them is no base
__device__ __forceinline__ bool ks_anchor(const uint8_t* __restrict__ bytes, uint64_t at, uint32_t k, uint64_t& fwd, uint64_t& rc) {
    fwd = rc = 0;
    bool ok = true;
    for (uint32_t i = 0; i < k; ++i) {
        const uint32_t c = base_code(bytes[at + i]);
        ok = ok && c < 4;
        fwd = (fwd << 2) | (c & 3u);
        rc = (rc >> 2) | ((uint64_t)(3u - (c & 3u)) << (2 * (k - 1)));
    }
    return ok;
}

template <bool MIN>
__device__ __forceinline__ void ks_walks_body(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ from, const uint64_t* __restrict__ to,
                                              const uint32_t* __restrict__ dlo, const uint32_t* __restrict__ dhi, uint32_t n_sites, uint32_t budget,
                                              uint32_t k, const uint64_t* __restrict__ table, uint64_t slots, uint32_t* __restrict__ status,
                                              uint32_t* __restrict__ steps_out, uint32_t* __restrict__ len_out, uint8_t* __restrict__ walk,
                                              const uint8_t* __restrict__ counts, uint32_t t) {
    __shared__ uint8_t stacks[KS_WALK_SITES * KS_WALK_STACK];
    const uint32_t lane = threadIdx.x & 63, b = lane & (KS_WALK_LANES - 1), gshift = lane & ~(uint32_t)(KS_WALK_LANES - 1);
    const uint64_t site = ((uint64_t)blockIdx.x * KS_THREADS + threadIdx.x) / KS_WALK_LANES;
    uint8_t* const stack = stacks + (threadIdx.x / KS_WALK_LANES) * KS_WALK_STACK;
    const bool have = site < n_sites;
    const uint64_t mask = (1ull << (2 * k)) - 1;
    const uint32_t rsh = 2 * (k - 1);
    uint64_t lf = 0, lr = 0, rf = 0, rr = 0, fwd = 0, rc = 0;
    uint32_t lo = 0, hi = 0, st = KS_WALK_NONE, steps = 0, found = 0, len = 0, d = 0;
    bool done = true, expand = false;
    if (have) {
        lo = dlo[site]; hi = dhi[site];
        const bool ok_l = ks_anchor(bytes, from[site], k, lf, lr), ok_r = ks_anchor(bytes, to[site], k, rf, rr);
        if (ok_l && ok_r) { done = false; expand = true; steps = 1; fwd = lf; rc = lr; }     // the visit of L: depth 0 < dlo, no arrival
        else st = KS_WALK_NOANCHOR;
    }
    while (__any(!done)) {
        // the groups that stepped onto a k-mer: which of its children does the set hold?
        bool hit = false;
        if (!done && expand) {
            const uint64_t yf = ((fwd << 2) | b) & mask, yr = (rc >> 2) | ((uint64_t)(3u - b) << rsh);
            const uint64_t key = yf < yr ? yf : yr;
            hit = MIN ? ks_contains_min(table, slots, counts, key, t) : ks_contains(table, slots, key);
        }
        const uint32_t kids = (uint32_t)(__ballot(hit) >> gshift) & 15u;
        if (done) continue;
        if (expand) { stack[d] = (uint8_t)kids; expand = false; }
        const uint32_t m = stack[d] & 15u;
        if (!m) {                                               // every child tried: one step back, or the search is over
            if (!d) { done = true; continue; }
            const uint32_t i = d - 1;                           // the base that fell off when the group stepped here: base i of L + path
            const uint32_t c = i < k ? (uint32_t)(lf >> (2 * (k - 1 - i))) & 3u : ((uint32_t)stack[i - k] >> 4) & 3u;
            fwd = (fwd >> 2) | ((uint64_t)c << rsh);
            rc = ((rc << 2) | (3u - c)) & mask;
            d = i;
            continue;
        }
        const uint32_t c = (uint32_t)__ffs(m) - 1;
        stack[d] = (uint8_t)((m & (m - 1)) | (c << 4));
        const uint64_t yf = ((fwd << 2) | c) & mask;
        if (++steps > budget) { st = KS_WALK_BUDGET; done = true; continue; }
        if (d + 1 >= lo && yf == rf) {                           // an arrival ends the walk
            if (++found == 2) { st = KS_WALK_AMBIGUOUS; done = true; continue; }
            len = d + 1;
            for (uint32_t x = b; x < len; x += KS_WALK_LANES) walk[site * KSET_MAX_WALK + x] = (uint8_t)ks_base_char(((uint32_t)stack[x] >> 4) & 3u);
            continue;
        }
        if (d + 1 == hi) continue;
        fwd = yf; rc = (rc >> 2) | ((uint64_t)(3u - c) << rsh);
        ++d; expand = true;
    }
    if (have && b == 0) {
        if (st == KS_WALK_NONE && found) st = KS_WALK_UNIQUE;
        if (st == KS_WALK_BUDGET) len = 0;
        status[site] = st; steps_out[site] = steps; len_out[site] = len;
    }
}

__global__ void __launch_bounds__(KS_THREADS) kset_walks_kernel(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ from,
                                                                 const uint64_t* __restrict__ to, const uint32_t* __restrict__ dlo,
                                                                 const uint32_t* __restrict__ dhi, uint32_t n_sites, uint32_t budget, uint32_t k,
                                                                 const uint64_t* __restrict__ table, uint64_t slots, uint32_t* __restrict__ status,
                                                                 uint32_t* __restrict__ steps, uint32_t* __restrict__ len, uint8_t* __restrict__ walk) {
    ks_walks_body<false>(bytes, from, to, dlo, dhi, n_sites, budget, k, table, slots, status, steps, len, walk, nullptr, 1);
}

// kset_walks_kernel against R_t (hypo --qv-min-count; the section "a least count" above)
__global__ void __launch_bounds__(KS_THREADS) kset_walks_min_kernel(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ from,
                                                                     const uint64_t* __restrict__ to, const uint32_t* __restrict__ dlo,
                                                                     const uint32_t* __restrict__ dhi, uint32_t n_sites, uint32_t budget, uint32_t k,
                                                                     const uint64_t* __restrict__ table, uint64_t slots, uint32_t* __restrict__ status,
                                                                     uint32_t* __restrict__ steps, uint32_t* __restrict__ len, uint8_t* __restrict__ walk,
                                                                     const uint8_t* __restrict__ counts, uint32_t t) {
    ks_walks_body<true>(bytes, from, to, dlo, dhi, n_sites, budget, k, table, slots, status, steps, len, walk, counts, t);
}

hipError_t kset_walks_run(const KsetView& set, const KsetWalkSites& s, uint32_t budget, uint32_t* status, uint32_t* steps, uint32_t* len, uint8_t* walk,
                          hipStream_t st) {
    if (!s.n_sites) return hipSuccess;
    static_assert(KSET_MAX_WALK <= KS_WALK_STACK, "a stack byte per depth");
    const uint32_t blocks = (s.n_sites + KS_WALK_SITES - 1) / KS_WALK_SITES;
    if (set.min_count > 1)
        kset_walks_min_kernel<<<dim3(blocks), dim3(KS_THREADS), 0, st>>>(s.bytes, s.from, s.to, s.dlo, s.dhi, s.n_sites, budget, set.k, set.table, set.slots, status, steps, len,
                                                                         walk, (const uint8_t*)set.planes, set.min_count);
    else
        kset_walks_kernel<<<dim3(blocks), dim3(KS_THREADS), 0, st>>>(s.bytes, s.from, s.to, s.dlo, s.dhi, s.n_sites, budget, set.k, set.table, set.slots, status, steps, len, walk);
    return hipGetLastError();
}

// ---- up to four walks between two anchors, each with its support (hypo --kmer-bridge-vote; DESIGN.md "k-mer bridge vote") -------------
// The search of kset_walks_kernel, not stopped at the second arrival: it goes on until the tree is exhausted, a fifth walk arrives
// (MANY) or the budget is spent, and every walk that arrives is written into the site's next slot with its length and its `low`,
// the least count byte among the k-mers at its depths 1 .. len (R included, L not).  A child exists iff its count byte is at least
// t (t = 1: iff the set holds it; an absent key counts 0), so one kernel serves every t.  The geometry, the ballot, the stack byte
// per depth and the rebuilt parent are the sibling's.
// The running minimum: the count of the child a group steps onto was loaded by another lane in an earlier iteration, so the group
// asks again.  In the iteration that expands the k-mer x at depth d >= 1 all four lanes also probe x itself (one address for the
// group, issued with the child probes) and store lowmin[d] = min(lowmin[d - 1], count(x)) in a second LDS byte per depth;
// lowmin[0] = 255 (L is not counted).  count(R) is loaded once per site, and an arrival from depth d has low = min(lowmin[d],
// count(R)).  As with the stack, every lane of a group stores and loads the same bytes.  2 * 260 bytes a site, 33 280 a workgroup.
// Bounds: a site makes at most `budget` <= KSET_MAX_WALK_BUDGET visits and no more steps back than visits, so the loop ends after
// at most 2 budget + 2 iterations; a probe takes at most `slots` steps, an expansion makes two of them and a site one more for R;
// depth <= dhi <= KSET_MAX_WALK = 256, stack and lowmin are indexed at depth < dhi (a k-mer at depth dhi is never expanded; d - 1
// only with d >= 1), below KS_WALK_STACK; a walk is written only while found < KSET_WALK_SETS, at slot = s * 4 + found < n_sites * 4:
// len / low at [slot], walk[] at [slot * 256, slot * 256 + len), len <= dhi; counts[] at a slot ks_find returned, < slots; bytes
// are read at [from, from + k) and [to, to + k), which the caller checked to lie inside the text; status / steps / n_walks are
// indexed below n_sites.
enum { KS_WALK_MANY = 5 };

// the count byte of the key, 0 when the set does not hold it
__device__ __forceinline__ uint32_t ks_count_of(const uint64_t* __restrict__ table, uint64_t slots, const uint8_t* __restrict__ counts, uint64_t key) {
    const uint64_t s = ks_find(table, slots, key);
    return s == KSET_EMPTY ? 0u : (uint32_t)counts[s];
}

__global__ void __launch_bounds__(KS_THREADS) kset_walk_sets_kernel(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ from,
                                                                     const uint64_t* __restrict__ to, const uint32_t* __restrict__ dlo,
                                                                     const uint32_t* __restrict__ dhi, uint32_t n_sites, uint32_t budget, uint32_t k,
                                                                     const uint64_t* __restrict__ table, uint64_t slots, const uint8_t* __restrict__ counts,
                                                                     uint32_t t, uint32_t* __restrict__ status, uint32_t* __restrict__ steps_out,
                                                                     uint32_t* __restrict__ n_walks, uint32_t* __restrict__ len_out,
                                                                     uint32_t* __restrict__ low_out, uint8_t* __restrict__ walk) {
    __shared__ uint8_t stacks[KS_WALK_SITES * KS_WALK_STACK];
    __shared__ uint8_t lowmins[KS_WALK_SITES * KS_WALK_STACK];
    const uint32_t lane = threadIdx.x & 63, b = lane & (KS_WALK_LANES - 1), gshift = lane & ~(uint32_t)(KS_WALK_LANES - 1);
    const uint64_t site = ((uint64_t)blockIdx.x * KS_THREADS + threadIdx.x) / KS_WALK_LANES;
    uint8_t* const stack = stacks + (threadIdx.x / KS_WALK_LANES) * KS_WALK_STACK;
    uint8_t* const lowmin = lowmins + (threadIdx.x / KS_WALK_LANES) * KS_WALK_STACK;
    const bool have = site < n_sites;
    const uint64_t mask = (1ull << (2 * k)) - 1;
    const uint32_t rsh = 2 * (k - 1);
    uint64_t lf = 0, lr = 0, rf = 0, rr = 0, fwd = 0, rc = 0;
    uint32_t lo = 0, hi = 0, st = KS_WALK_NONE, steps = 0, found = 0, d = 0, cr = 0;
    bool done = true, expand = false;
    if (have) {
        lo = dlo[site]; hi = dhi[site];
        const bool ok_l = ks_anchor(bytes, from[site], k, lf, lr), ok_r = ks_anchor(bytes, to[site], k, rf, rr);
        if (ok_l && ok_r) {                                      // the visit of L: depth 0 < dlo, no arrival
            done = false; expand = true; steps = 1; fwd = lf; rc = lr;
            cr = ks_count_of(table, slots, counts, rf < rr ? rf : rr);
        } else st = KS_WALK_NOANCHOR;
    }
    while (__any(!done)) {
        // the groups that stepped onto a k-mer: the counts of its children, and its own
        uint32_t cy = 0, cx = 255;
        if (!done && expand) {
            const uint64_t yf = ((fwd << 2) | b) & mask, yr = (rc >> 2) | ((uint64_t)(3u - b) << rsh);
            cy = ks_count_of(table, slots, counts, yf < yr ? yf : yr);
            if (d) cx = ks_count_of(table, slots, counts, fwd < rc ? fwd : rc);
        }
        const uint32_t kids = (uint32_t)(__ballot(cy >= t) >> gshift) & 15u;
        if (done) continue;
        if (expand) {
            const uint32_t up = d ? (uint32_t)lowmin[d - 1] : 255u;
            stack[d] = (uint8_t)kids; lowmin[d] = (uint8_t)(cx < up ? cx : up); expand = false;
        }
        const uint32_t m = stack[d] & 15u;
        if (!m) {                                               // every child tried: one step back, or the search is over
            if (!d) { done = true; continue; }
            const uint32_t i = d - 1;                           // the base that fell off when the group stepped here: base i of L + path
            const uint32_t c = i < k ? (uint32_t)(lf >> (2 * (k - 1 - i))) & 3u : ((uint32_t)stack[i - k] >> 4) & 3u;
            fwd = (fwd >> 2) | ((uint64_t)c << rsh);
            rc = ((rc << 2) | (3u - c)) & mask;
            d = i;
            continue;
        }
        const uint32_t c = (uint32_t)__ffs(m) - 1;
        stack[d] = (uint8_t)((m & (m - 1)) | (c << 4));
        const uint64_t yf = ((fwd << 2) | c) & mask;
        if (++steps > budget) { st = KS_WALK_BUDGET; done = true; continue; }
        if (d + 1 >= lo && yf == rf) {                           // an arrival ends the walk
            if (found == KSET_WALK_SETS) { st = KS_WALK_MANY; done = true; continue; }
            const uint64_t slot = site * KSET_WALK_SETS + found;
            const uint32_t len = d + 1, up = lowmin[d];
            if (b == 0) { len_out[slot] = len; low_out[slot] = cr < up ? cr : up; }
            for (uint32_t x = b; x < len; x += KS_WALK_LANES) walk[slot * KSET_MAX_WALK + x] = (uint8_t)ks_base_char(((uint32_t)stack[x] >> 4) & 3u);
            ++found;
            continue;
        }
        if (d + 1 == hi) continue;
        fwd = yf; rc = (rc >> 2) | ((uint64_t)(3u - c) << rsh);
        ++d; expand = true;
    }
    if (have && b == 0) {
        if (st == KS_WALK_NONE && found) st = found == 1 ? KS_WALK_UNIQUE : KS_WALK_AMBIGUOUS;
        status[site] = st; steps_out[site] = steps; n_walks[site] = st == KS_WALK_BUDGET || st == KS_WALK_NOANCHOR ? 0u : found;
    }
}

hipError_t kset_walk_sets_run(const KsetView& set, const KsetWalkSites& s, uint32_t budget, uint32_t* status, uint32_t* steps, uint32_t* n_walks,
                              uint32_t* len, uint32_t* low, uint8_t* walk, hipStream_t st) {
    if (!s.n_sites) return hipSuccess;
    const uint32_t blocks = (s.n_sites + KS_WALK_SITES - 1) / KS_WALK_SITES;
    kset_walk_sets_kernel<<<dim3(blocks), dim3(KS_THREADS), 0, st>>>(s.bytes, s.from, s.to, s.dlo, s.dhi, s.n_sites, budget, set.k, set.table, set.slots,
                                                                     (const uint8_t*)set.planes, set.min_count < 1 ? 1u : set.min_count, status, steps, n_walks, len, low, walk);
    return hipGetLastError();
}

hipError_t kset_insert_run(const uint8_t* bytes, uint64_t n, uint32_t k, uint64_t* table, uint64_t slots, unsigned long long* ctr, hipStream_t st) {
    if (!n) return hipSuccess;
    const uint64_t blocks = (n + KR_BLOCK_BYTES - 1) / KR_BLOCK_BYTES;
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

uint64_t ks_plane_words(uint64_t slots) { return ((slots + 255) / 256) * 64; }

hipError_t kset_insert_count_run(const uint8_t* bytes, uint64_t n, uint32_t k, uint64_t* table, uint64_t slots, unsigned long long* ctr,
                                 uint32_t* planes, hipStream_t st) {
    if (!n) return hipSuccess;
    const uint64_t blocks = (n + KR_BLOCK_BYTES - 1) / KR_BLOCK_BYTES;
    kset_insert_count_kernel<<<dim3((uint32_t)blocks), dim3(KS_THREADS), 0, st>>>(bytes, n, k, table, slots, ctr, planes);
    return hipGetLastError();
}

hipError_t kset_rehash_count_run(const uint64_t* old_table, uint64_t old_slots, const uint32_t* old_planes, uint64_t* table, uint64_t slots,
                                 uint32_t* planes, unsigned long long* ctr, hipStream_t st) {
    if (!old_slots) return hipSuccess;
    uint64_t blocks = (old_slots + KS_THREADS - 1) / KS_THREADS;
    if (blocks > 16384) blocks = 16384;
    kset_rehash_count_kernel<<<dim3((uint32_t)blocks), dim3(KS_THREADS), 0, st>>>(old_table, old_slots, table, slots, ctr, (const uint8_t*)old_planes,
                                                                                  (uint8_t*)planes);
    return hipGetLastError();
}

hipError_t kset_mark_run(const uint8_t* bytes, const uint64_t* off, uint32_t n_seqs, uint64_t n, uint32_t k, const uint64_t* table, uint64_t slots,
                         uint32_t* planes, uint32_t text, unsigned long long* sums, hipStream_t st) {
    if (!n || !n_seqs) return hipSuccess;
    const uint64_t blocks = (n + KR_BLOCK_BYTES - 1) / KR_BLOCK_BYTES;
    kset_mark_kernel<<<dim3((uint32_t)blocks), dim3(KS_THREADS), 0, st>>>(bytes, off, n_seqs, n, k, table, slots, planes + (1 + (uint64_t)text) * ks_plane_words(slots), sums);
    return hipGetLastError();
}

hipError_t kset_spectrum_run(const uint32_t* planes, uint64_t slots, uint32_t text, unsigned long long* hist, hipStream_t st) {
    const uint64_t n_words = ks_plane_words(slots);
    uint64_t blocks = (n_words + KS_THREADS - 1) / KS_THREADS;
    if (blocks > 4096) blocks = 4096;
    kset_spectrum_kernel<<<dim3((uint32_t)blocks), dim3(KS_THREADS), 0, st>>>(planes, planes + (1 + (uint64_t)text) * n_words, n_words, hist);
    return hipGetLastError();
}

hipError_t kset_query_run(const KsetView& set, const uint8_t* bytes, const uint64_t* off, uint32_t n_seqs, uint64_t n, unsigned long long* total,
                          unsigned long long* missing, hipStream_t st) {
    if (!n || !n_seqs) return hipSuccess;
    const uint64_t blocks = (n + KR_BLOCK_BYTES - 1) / KR_BLOCK_BYTES;
    if (set.min_count > 1)
        kset_query_min_kernel<<<dim3((uint32_t)blocks), dim3(KS_THREADS), 0, st>>>(bytes, off, n_seqs, n, set.k, set.table, set.slots, total, missing,
                                                                                   (const uint8_t*)set.planes, set.min_count);
    else kset_query_kernel<<<dim3((uint32_t)blocks), dim3(KS_THREADS), 0, st>>>(bytes, off, n_seqs, n, set.k, set.table, set.slots, total, missing);
    return hipGetLastError();
}

// ---- the set's records out of the table and back in (hypo --qv-save / --qv-load; DESIGN.md "k-mer set file") ------------------------
// A record is a key as the table holds it and its count byte (1 on a set that keeps no counts).  The digest of a record is
// mix64(key) + count * KS_DIGEST_MUL mod 2^64, that of a list the sum over its records: integers, so the order of the sum is free.
// Export is an ordered stream compaction of the slot range [s0, s0 + n_slots), s0 + n_slots <= slots, which the host bounds to the
// caller's `cap`: a range never holds more keys than slots.  A workgroup owns a tile of KS_THREADS consecutive slots of the range,
// a lane one slot; lanes of the last tile beyond the range own nothing.
//   * kset_export_count_kernel: the occupied slots of every tile, one plain store per workgroup.
//   * kset_export_scan_kernel: ONE workgroup turns the tile sums into exclusive prefixes, KS_SCAN_THREADS of them per pass (the pattern of
//     kset_track_scan_kernel with one field), and leaves the range's total behind the last one.
//   * kset_export_emit_kernel: the same loads again; a lane's rank is the prefix of its tile, the occupied slots of the waves before
//     its own (through LDS) and those of the lanes before it (a ballot and a popcount), so the records come in ascending slot order
//     and the arrays are a function of the table alone.  Keys are stored as 8-byte values, counts as bytes.  The digests are summed
//     per wave and added once per wave.
// No kernel waits for another workgroup and none loops over slots.  Bounds: slots are read at s0 + i for i < n_slots only (the host
// checked s0 + n_slots <= slots), count bytes at the same indices of a plane of ks_plane_words(slots) * 4 >= slots bytes; tile sums
// below n_tiles = gridDim.x of the count and emit kernels, prefixes below n_tiles + 1; records below `cap` (checked per store; the
// host passes cap >= n_slots).  Loops: scan passes = ceil(n_tiles / KS_SCAN_THREADS), the waves of a workgroup.
constexpr uint64_t KS_DIGEST_MUL = 0x9e3779b97f4a7c15ull;

__device__ __forceinline__ uint64_t ks_wave_sum64(uint64_t v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ void __launch_bounds__(KS_THREADS) kset_export_count_kernel(const uint64_t* __restrict__ table, uint64_t s0, uint64_t n_slots,
                                                                        uint64_t* __restrict__ sums) {
    __shared__ uint32_t part[KS_THREADS / 64];
    const uint64_t i = (uint64_t)blockIdx.x * KS_THREADS + threadIdx.x;
    const bool used = i < n_slots && table[s0 + i] != KSET_EMPTY;
    const uint32_t n = (uint32_t)__popcll(__ballot(used));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) sums[blockIdx.x] = (uint64_t)part[0] + part[1] + part[2] + part[3];
}

// pre[t]: the occupied slots of the tiles before t; pre[n_tiles]: those of the range
__global__ void __launch_bounds__(KS_SCAN_THREADS) kset_export_scan_kernel(const uint64_t* __restrict__ sums, uint32_t n_tiles, uint64_t* __restrict__ pre) {
    constexpr int WAVES = KS_SCAN_THREADS / 64;
    __shared__ uint64_t part[WAVES];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint64_t carry = 0;
    for (uint32_t base = 0; base < n_tiles; base += KS_SCAN_THREADS) {
        const uint32_t i = base + threadIdx.x;
        const uint64_t v = i < n_tiles ? sums[i] : 0;
        const uint64_t inc = ks_wave_inclusive(v);
        if (lane == 63) part[wave] = inc;
        __syncthreads();
        uint64_t before = carry, all = 0;
        for (int x = 0; x < WAVES; ++x) { const uint64_t t = part[x]; if ((uint32_t)x < wave) before += t; all += t; }
        if (i < n_tiles) pre[i] = before + inc - v;
        carry += all;
        __syncthreads();                                        // (part is written again in the next pass)
    }
    if (threadIdx.x == 0) pre[n_tiles] = carry;
}

// counts: plane 0 as bytes, or NULL (every count is 1); out_counts: NULL when the caller wants none; digest: one 64-bit sum
__global__ void __launch_bounds__(KS_THREADS) kset_export_emit_kernel(const uint64_t* __restrict__ table, const uint8_t* __restrict__ counts, uint64_t s0,
                                                                       uint64_t n_slots, const uint64_t* __restrict__ pre, uint64_t cap,
                                                                       uint64_t* __restrict__ out_keys, uint8_t* __restrict__ out_counts,
                                                                       unsigned long long* digest) {
    __shared__ uint32_t part[KS_THREADS / 64];
    const uint64_t i = (uint64_t)blockIdx.x * KS_THREADS + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t key = i < n_slots ? table[s0 + i] : KSET_EMPTY;
    const bool used = key != KSET_EMPTY;
    const uint32_t c = used && counts ? counts[s0 + i] : 1u;
    const uint64_t mask = __ballot(used);
    if (lane == 0) part[wave] = (uint32_t)__popcll(mask);
    __syncthreads();
    uint64_t rank = pre[blockIdx.x] + (uint64_t)__popcll(mask & ((1ull << lane) - 1ull));
    for (uint32_t x = 0; x < wave; ++x) rank += part[x];
    if (used && rank < cap) {
        out_keys[rank] = key;
        if (out_counts) out_counts[rank] = (uint8_t)c;
    }
    const uint64_t d = ks_wave_sum64(used ? ks_mix64(key) + (uint64_t)c * KS_DIGEST_MUL : 0ull);
    if (lane == 0 && mask) atomicAdd(digest, (unsigned long long)d);
}

// Import: n records handed in as two arrays.  kset_import_check_kernel looks at all of them before the table is touched, and
// kset_import_kernel puts them in: a lane per record in a grid-stride loop (keys are loaded coalesced), ks_insert<true> for the
// slot, and on a set that counts ks_byte_add for the count byte.  The same key twice in a call, in neighbouring lanes or not, is
// two adds to one byte.
//   * a record is refused when its key is not below 4^k, is greater than its reverse complement (not canonical), or its count byte
//     is 0: a wave that holds one takes the least index among its lanes and lowers bad[1] to it with ONE atomic, and stores 1 in
//     bad[0] (the same value from every wave).  bad[1] starts as all-ones, so it ends as the least refused index of the call.
//   * new keys (32 bits a lane: a lane sees at most ceil(n / lanes of the grid) < 2^32 records) and digests are summed per wave and
//     added once per wave.
// Bounds: keys / counts are read below n; slots as ks_insert says (at most `slots` steps, the overflow flag looked at every 64); the
// byte of a slot < slots in a plane of ks_plane_words(slots) words.  Loops: grid-stride, ceil(n / lanes of the grid) rounds.
__device__ __forceinline__ uint64_t ks_revcomp(uint64_t key, uint32_t k) {     // of a code below 4^k
    uint64_t x = ~key;                                          // (the bits above 2k turn to ones and leave at the low end)
    x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
    x = ((x >> 4) & 0x0f0f0f0f0f0f0f0full) | ((x & 0x0f0f0f0f0f0f0f0full) << 4);
    return __builtin_bswap64(x) >> (64 - 2 * k);
}

// ks_byte_inc adding v = 1..255: byte `slot` of `plane` becomes min(255, byte + v).  The same compare-and-swap loop: the lane loads
// first and does nothing once the byte reads 255; saturation is decided on the value the atomic returned, the new word differs
// from that value in this slot's byte only, and it is only ever swapped in against the word it was made from, so no byte wraps and
// no neighbour is touched.  Lock-free: a swap fails only because another lane's went through, every swap that goes through raises
// a byte of the word by at least 1, and a word takes at most 4 * 255 of them: at most 1021 rounds whatever the input is.
// Bounds: slot < slots, and a plane has ks_plane_words(slots) words.
__device__ __forceinline__ void ks_byte_add(uint32_t* plane, uint64_t slot, uint32_t v) {
    uint32_t* w = plane + (slot >> 2);
    const uint32_t sh = 8u * (uint32_t)(slot & 3);
    uint32_t cur = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (;;) {
        const uint32_t b = (cur >> sh) & 0xffu;
        if (b == 0xffu) return;
        const uint32_t nb = b + v < 0xffu ? b + v : 0xffu;
        const uint32_t prev = atomicCAS(w, cur, (cur & ~(0xffu << sh)) | (nb << sh));
        if (prev == cur) return;
        cur = prev;
    }
}

__global__ void __launch_bounds__(KS_THREADS) kset_import_check_kernel(const uint64_t* __restrict__ keys, const uint8_t* __restrict__ counts, uint64_t n,
                                                                        uint32_t k, unsigned long long* bad) {
    const uint64_t stride = (uint64_t)gridDim.x * KS_THREADS;
    const uint64_t end = 1ull << (2 * k);
    unsigned long long first = ~0ull;                           // the least refused index this lane has seen
    for (uint64_t i = (uint64_t)blockIdx.x * KS_THREADS + threadIdx.x; i < n; i += stride) {
        const uint64_t key = keys[i];
        if ((key >= end || key > ks_revcomp(key, k) || (counts && counts[i] == 0)) && i < first) first = i;
    }
    for (int o = 32; o > 0; o >>= 1) { const unsigned long long u = __shfl_xor(first, o); if (u < first) first = u; }
    if ((threadIdx.x & 63) == 0 && first != ~0ull) { atomicMin(bad + 1, first); bad[0] = 1ull; }
}

// plane: the count plane of a set that counts, or NULL; counts: NULL = 1 each; ctr as for kset_insert_kernel
__global__ void __launch_bounds__(KS_THREADS) kset_import_kernel(const uint64_t* __restrict__ keys, const uint8_t* __restrict__ counts, uint64_t n,
                                                                  uint64_t* table, uint64_t slots, unsigned long long* ctr, uint32_t* plane,
                                                                  unsigned long long* digest) {
    const uint64_t stride = (uint64_t)gridDim.x * KS_THREADS;
    uint32_t n_new = 0;
    uint64_t d = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * KS_THREADS + threadIdx.x; i < n; i += stride) {
        const uint64_t key = keys[i];
        const uint32_t c = counts ? counts[i] : 1u;
        uint64_t at;
        n_new += ks_insert<true>(table, slots, key, ctr, &at);
        if (plane && at != KSET_EMPTY) ks_byte_add(plane, at, c);
        d += ks_mix64(key) + (uint64_t)c * KS_DIGEST_MUL;
    }
    ks_wave_add(ctr, n_new);
    d = ks_wave_sum64(d);
    if ((threadIdx.x & 63) == 0 && d) atomicAdd(digest, (unsigned long long)d);
}

uint32_t kset_export_tiles(uint64_t n_slots) { return (uint32_t)((n_slots + KS_THREADS - 1) / KS_THREADS); }

hipError_t kset_export_run(const uint64_t* table, const uint32_t* planes, uint64_t s0, uint64_t n_slots, uint64_t* sums, uint64_t* pre, uint64_t cap,
                           uint64_t* out_keys, uint8_t* out_counts, unsigned long long* digest, hipStream_t st) {
    if (!n_slots) return hipSuccess;
    const uint32_t tiles = kset_export_tiles(n_slots);
    kset_export_count_kernel<<<dim3(tiles), dim3(KS_THREADS), 0, st>>>(table, s0, n_slots, sums);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    kset_export_scan_kernel<<<dim3(1), dim3(KS_SCAN_THREADS), 0, st>>>(sums, tiles, pre);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    kset_export_emit_kernel<<<dim3(tiles), dim3(KS_THREADS), 0, st>>>(table, (const uint8_t*)planes, s0, n_slots, pre, cap, out_keys, out_counts, digest);
    return hipGetLastError();
}

hipError_t kset_import_check_run(const uint64_t* keys, const uint8_t* counts, uint64_t n, uint32_t k, unsigned long long* bad, hipStream_t st) {
    if (!n) return hipSuccess;
    uint64_t blocks = (n + KS_THREADS - 1) / KS_THREADS;
    if (blocks > 16384) blocks = 16384;
    kset_import_check_kernel<<<dim3((uint32_t)blocks), dim3(KS_THREADS), 0, st>>>(keys, counts, n, k, bad);
    return hipGetLastError();
}

hipError_t kset_import_run(const uint64_t* keys, const uint8_t* counts, uint64_t n, uint64_t* table, uint64_t slots, unsigned long long* ctr,
                           uint32_t* planes, unsigned long long* digest, hipStream_t st) {
    if (!n) return hipSuccess;
    uint64_t blocks = (n + KS_THREADS - 1) / KS_THREADS;
    if (blocks > 16384) blocks = 16384;
    kset_import_kernel<<<dim3((uint32_t)blocks), dim3(KS_THREADS), 0, st>>>(keys, counts, n, table, slots, ctr, planes, digest);
    return hipGetLastError();
}

// ---- read count against copy number, bin by bin (hypo --qv-cn; DESIGN.md "k-mer copy number") ----------------------------------------
// A bin is `bin` consecutive window STARTS of one sequence; a bin never crosses a sequence, and bin_off[s] = the bins of the sequences
// before s (bin_off[n_seqs] = n_bins), so the sequence of bin b is ks_seq_of(bin_off, n_seqs, b).  One wave owns one bin, a workgroup
// four of them: nothing is summed across waves and no atomic touches global memory.
//   * The wave walks its bin in passes of 64 stretches.  A lane's stretch is `per` consecutive starts, per = ceil(starts / 64) capped
//     at KS_DEPTH_STRETCH: a bin of up to 64 * KS_DEPTH_STRETCH starts is one pass with every lane at work, a larger one loops.  The lane
//     rolls fwd / rc over the per + k - 1 bytes of its stretch (KmerRoll: any byte other than ACGTacgt restarts the run, and a run that
//     starts at the stretch's first byte yields only windows that start in the stretch), probes with ks_find, and loads the slot's
//     count byte c and, for a present window (c >= t), its copy byte m of the text plane.
//   * Present windows bump the wave's own 256 x 32-bit histogram of c in LDS (1 KiB a wave).  windows / missing / rated / over /
//     under are lane counters, summed over the wave with shuffles.
//   * The lower median: lane l holds bins 4 l .. 4 l + 3, a wave-wide inclusive scan of the lanes' sums finds the one lane whose bins
//     reach the rank ceil(present / 2), and that lane walks its four bins.
// The work is the dependent probe loads, as in the other query kernels.  Lane 0 stores the bin's six values: a bin without a window
// gets zeros, and every bin below n_bins has a wave.  The answer is a function of the bytes, the planes and t alone.
// Bounds: a lane reads bytes[off[s] + lo + w0 + i], i < w1 - w0 + k - 1, with lo + w1 <= hi <= len - k + 1, so below off[s + 1] <= n;
// the two plane bytes of a slot < slots (a plane has ks_plane_words(slots) * 4 >= slots bytes); LDS bins at a byte, below 256; outputs
// at b < n_bins.  Loops: passes = ceil(starts / (64 * per)) <= bin / 64 + 1, a stretch's bytes <= KS_DEPTH_STRETCH + 30, probes <=
// slots, the search <= 32 steps.  The two barriers are reached by every lane: nothing between them leaves the kernel.
constexpr uint32_t KS_DEPTH_STRETCH = 32;
constexpr int KS_DEPTH_WAVES = KS_THREADS / 64;

__device__ __forceinline__ uint32_t ks_wave_sum32(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ void __launch_bounds__(KS_THREADS) kset_depth_kernel(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ off,
                                                                 const uint64_t* __restrict__ bin_off, uint32_t n_seqs, uint64_t n_bins, uint32_t bin,
                                                                 uint32_t k, const uint64_t* __restrict__ table, uint64_t slots,
                                                                 const uint8_t* __restrict__ counts, const uint8_t* __restrict__ copies, uint32_t t,
                                                                 uint32_t unit, KsetDepthOut out) {
    __shared__ __attribute__((aligned(16))) uint32_t hist[KS_DEPTH_WAVES][256];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint32_t* h = hist[wave];
    *(uint4*)(h + 4 * lane) = make_uint4(0, 0, 0, 0);
    __syncthreads();
    const uint64_t b = (uint64_t)blockIdx.x * KS_DEPTH_WAVES + wave;
    const bool have = b < n_bins;                               // (wave-uniform)
    uint32_t win = 0, mis = 0, rat = 0, ov = 0, un = 0;
    if (have) {
        const uint32_t s = ks_seq_of(bin_off, n_seqs, b);
        const uint64_t base = off[s], len = off[s + 1] - base;
        const uint64_t lo = (b - bin_off[s]) * bin;             // the bin's window starts: [lo, hi) of the sequence
        uint64_t hi = len >= k ? len - k + 1 : 0;
        if (hi > lo + bin) hi = lo + bin;
        const uint32_t n_starts = hi > lo ? (uint32_t)(hi - lo) : 0;
        uint32_t per = (n_starts + 63) / 64;
        per = per < 1 ? 1 : per > KS_DEPTH_STRETCH ? KS_DEPTH_STRETCH : per;
        const uint32_t um3 = 3 * unit;
        for (uint32_t p0 = 0; p0 < n_starts; p0 += 64 * per) {
            const uint32_t w0 = p0 + lane * per;
            if (w0 >= n_starts) continue;
            const uint32_t w1 = w0 + per < n_starts ? w0 + per : n_starts;
            const uint8_t* __restrict__ src = bytes + base + lo + w0;
            const uint32_t n_src = w1 - w0 + k - 1;
            KmerRoll roll(k);
            for (uint32_t i = 0; i < n_src; ++i) {
                if (!roll.push(src[i])) continue;
                ++win;
                const uint64_t at = ks_find(table, slots, roll.canon());
                const uint32_t c = at != KSET_EMPTY ? counts[at] : 0u;
                if (c < t) { ++mis; continue; }                 // (t >= 1: a k-mer the set does not hold is missing)
                atomicAdd(&h[c], 1u);
                const uint32_t m = copies[at];
                if (m >= 1 && m <= 254 && c <= 254) {           // (a saturated byte says "at least")
                    ++rat;
                    if (2 * c >= um3 * m) ++ov;
                    if (4 * c <= um3 * m) ++un;
                }
            }
        }
    }
    __syncthreads();
    win = ks_wave_sum32(win); mis = ks_wave_sum32(mis); rat = ks_wave_sum32(rat); ov = ks_wave_sum32(ov); un = ks_wave_sum32(un);
    const uint4 mine = *(const uint4*)(h + 4 * lane);
    const uint32_t sum = mine.x + mine.y + mine.z + mine.w;
    uint32_t inc = sum;
    for (int o = 1; o < 64; o <<= 1) { const uint32_t u = __shfl_up(inc, o); if (lane >= (uint32_t)o) inc += u; }
    const uint32_t present = __shfl(inc, 63), rank = (present + 1) / 2;
    uint32_t med = 256;
    if (present && inc - sum < rank && rank <= inc) {           // the one lane whose bins reach the rank
        uint32_t cum = inc - sum;
        med = 4 * lane;
        if ((cum += mine.x) < rank) { ++med; if ((cum += mine.y) < rank) { ++med; if ((cum += mine.z) < rank) ++med; } }
    }
    for (int o = 32; o > 0; o >>= 1) { const uint32_t u = __shfl_xor(med, o); if (u < med) med = u; }
    if (have && lane == 0) {
        out.windows[b] = win; out.missing[b] = mis; out.rated[b] = rat; out.over[b] = ov; out.under[b] = un;
        out.med_count[b] = (uint8_t)(present ? med : 0u);
    }
}

hipError_t kset_depth_run(const KsetView& set, const uint8_t* bytes, const uint64_t* off, const uint64_t* bin_off, uint32_t n_seqs, uint64_t n_bins,
                          uint32_t bin, uint32_t text, uint32_t unit, const KsetDepthOut& out, hipStream_t st) {
    if (!n_bins || !n_seqs) return hipSuccess;
    const uint64_t n_words = ks_plane_words(set.slots);
    const uint64_t blocks = (n_bins + KS_DEPTH_WAVES - 1) / KS_DEPTH_WAVES;
    kset_depth_kernel<<<dim3((uint32_t)blocks), dim3(KS_THREADS), 0, st>>>(bytes, off, bin_off, n_seqs, n_bins, bin, set.k, set.table, set.slots,
                                                                           (const uint8_t*)set.planes, (const uint8_t*)(set.planes + (1 + (uint64_t)text) * n_words),
                                                                           set.min_count > 1 ? set.min_count : 1u, unit, out);
    return hipGetLastError();
}

}  // namespace hypo
