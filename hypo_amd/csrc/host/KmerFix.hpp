// KmerFix.hpp — hypo --kmer-fix: one pass of single-base fixes over the text that would otherwise be written, made where the k-mers
// of the short reads pin an isolated error down (DESIGN.md "k-mer fix").  The intervals of missing k-mers of every text come from one
// track query of the reads' set on context 0 (ReadKmerSet::query_track).  An interval in which every window is missing, not longer
// than 2k - 1, at least k - 1 bases from its neighbours, whose span with the k - 1 bases on either side lies inside the contig and
// holds bases only, is a site; the positions all its missing windows share are its region.  Every substitution, deletion and
// insertion of one base in the region is asked by one hypo_gpu_kset_query_fixes call (kset_kernel.hip), and a site where exactly
// one of the distinct edited texts lacks no k-mer of the reads gets that edit.  Sites are at least k - 1 bases apart, so no window
// sees two fixes and a contig's missing k-mers drop by exactly the fixed intervals' counts.
#pragma once
#include <cstdint>
#include <functional>
#include <ostream>
#include <string>
#include <vector>
#include "ReadKmerSet.hpp"
#include "Settings.hpp"

namespace hypo {

class KmerFix {
public:
    struct Stats { uint64_t intervals = 0, sites = 0, fixed = 0, sub = 0, del = 0, ins = 0, ambiguous = 0, removed = 0; };
    // what a contig's turn hands on: the draft it came with and the fixed text
    using Emit = std::function<int(uint32_t contig, const std::string& draft, const std::string& text)>;

    explicit KmerFix(const ReadKmerSet& set) : _set(set) {}           // the set that is asked (its track query must be bound), and its k
    // binds hypo_gpu_kset_query_fixes by name (false: the device library does not provide it)
    bool bind();
    uint32_t k() const { return _set.k(); }
    // One contig's text (and its draft, which is only handed on).  The texts are asked on the calling thread's context when flush()
    // is called or enough text has gathered (at most ReadKmerSet::kTextPerCall a call; a larger contig gets a call of its own), and
    // `emit` gets every contig in the order they were pushed.  HYPO_OK, the C-ABI's error, or what emit answered.
    int push(uint32_t contig, const std::string& name, std::string draft, std::string text, const Emit& emit);
    int flush(const Emit& emit);
    const Stats& stats() const { return _stats; }
    // "#contig pos kind ref alt missing_kmers", one line per fix, contigs in the order they were pushed, pos ascending (0-based, in
    // the text before the fixes)
    void write(std::ostream& os) const;
private:
    const ReadKmerSet& _set;
    struct Pending { uint32_t contig = 0; std::string name, draft; uint64_t off = 0, len = 0; };
    int (*_fixes)(const char*, uint64_t, const uint64_t*, const uint64_t*, const uint64_t*, const uint64_t*, uint32_t, uint64_t*, uint64_t*, uint32_t*, uint64_t*,
                  uint64_t*, uint32_t*, uint64_t*, uint64_t*) = nullptr;
    Stats _stats;
    std::string _text;                                       // the texts of the pending contigs, back to back
    std::vector<Pending> _pending;
    std::string _lines;                                      // the TSV's lines so far
};

}  // namespace hypo
