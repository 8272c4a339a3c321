// kmer_kernel.hpp — host-visible interface of kmer_kernel.hip (internal to libhypo_gpu.so): canonical k-mer counting of
// short reads, the KMC-filtered histogram of the counts, and the solid 4^k-bit set (replaces KMC + suk::SolidKmers::initialise,
// external/suk/src/SolidKmers.cpp:68-208).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hypo {
// Counters saturate at `sat` (= 4c + 1, "above -cx"); `wide` = 2-byte counters (sat > 255), else 1 byte.
// table: 4^k counters indexed by the canonical code.  All pointers are device pointers.
hipError_t kmer_count_run(const uint8_t* bytes, uint64_t n, uint32_t k, void* table, int wide, uint32_t sat, hipStream_t st);
// hist[0 .. n_bins) (n_bins = sat), zeroed here: hist[v] += number of codes whose counter is v, for 2 <= v < sat.
hipError_t kmer_histogram_run(const void* table, uint32_t k, int wide, uint32_t n_bins, unsigned long long* hist, hipStream_t st);
// bits: 4^k / 64 words, every word written.  counts[0] = set bits, counts[1] = set canonical codes (code <= rc(code)), zeroed here.
hipError_t solid_fill_run(const void* table, uint32_t k, int wide, uint32_t lower, uint32_t upper, uint32_t sat, int exclude_hp,
                          uint64_t* bits, unsigned long long* counts, hipStream_t st);
}  // namespace hypo
