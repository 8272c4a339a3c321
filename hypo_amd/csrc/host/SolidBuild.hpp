// SolidBuild.hpp — the solid k-mer set built from the short reads (replaces suk::SolidKmers::initialise,
// external/suk/src/SolidKmers.cpp:68-208, called from src/Hypo.cpp:47-66).  Host part: the streaming read parser, the
// cut-offs (find_cutoffs restated), and the calls of the device path (hypo_gpu_kmer_*; kmer_kernel.hip).
#pragma once
#include <cstdint>
#include <functional>
#include <string>
#include <vector>
#include "Contig.hpp"

namespace hypo {

struct CutOffs { uint32_t err = 0, mean = 0, upper = 0, lower = 0; };    // suk::CutOffs (SolidKmers.hpp:69-74)

// suk::SolidKmers::find_cutoffs (SolidKmers.cpp:258-363), integer widths included; hist = hist[0 .. 4c].  false: the histogram has
// no maximum after the error threshold (the reference leaves CutOffs::mean unset there: undefined behaviour).
bool find_cutoffs(const std::vector<uint64_t>& hist, CutOffs& out);

struct SolidBuildStats {
    CutOffs cut;
    std::vector<uint64_t> hist;               // 4c + 1 bins
    uint64_t n_bits = 0, n_canonical = 0;
    uint64_t seq_bytes = 0, file_bytes = 0;   // bytes handed to the device, bytes of the (inflated) read files
    double parse_s = 0, count_s = 0, hist_s = 0, fill_s = 0, total_s = 0;
    double sink_s = 0;                        // inside the second consumer's add calls
};

enum { SOLID_OK = 0, SOLID_E_INPUT = 1, SOLID_E_UNDEFINED = 2, SOLID_E_DEVICE = 3, SOLID_E_K = 4, SOLID_E_SINK = 5 };

// An optional second consumer of the sequence bytes the parser produces (hypo --qv: the exact k-mer set of the reads, k-mers of
// length k).  add(bytes, n) follows hypo_gpu_kmer_count_add's rules and returns HYPO_OK or a C-ABI error (-> SOLID_E_SINK, `err` =
// hypo_gpu_last_error()).  Consecutive chunks overlap by at least k - 1 bytes.
// exact: the sink counts windows, so it gets each chunk from its own k - 1 bytes before the new ones (a window in two chunks would
// count twice); otherwise it gets the whole chunk, whose overlap may be longer when the solid k-mers are longer than its own.
struct ReadSink { uint32_t k = 0; std::function<int(const char*, uint64_t)> add; bool exact = false; };

// Counts the k-mers of `files` (FASTA / FASTQ, plain or gzip) on the calling thread's device context, picks the cut-offs, prints
// the reference's cut-offs line and "Number of solid kmers found" line, and fills sk (words, num_solid = canonical count).
// `threads`: host threads for the parser (gzip members are inflated by zlib on one of them).  Returns SOLID_*; `err` says why.
// `sink`: every chunk handed to the count table goes to it as well (one parse pass for both).
int build_solid_kmers(const std::vector<std::string>& files, uint32_t k, uint32_t coverage, int threads, SolidKmers& sk,
                      SolidBuildStats& stats, std::string& err, ReadSink* sink = nullptr);
// The same parse pass for the sink alone (a run that loads its solid k-mers from aux/ and still needs the reads' k-mer set).
int stream_reads(const std::vector<std::string>& files, ReadSink& sink, SolidBuildStats& stats, std::string& err);

}  // namespace hypo
