// KmerBridge.hpp — hypo --kmer-bridge: one pass of local reassembly over the text that would otherwise be written (after --kmer-guard
// and --kmer-fix), where the k-mers of the short reads spell exactly one other text between two k-mers they do contain (DESIGN.md
// "k-mer bridge").  The intervals of missing k-mers of every text come from one track query of the reads' set on context 0
// (ReadKmerSet::query_track).  An interval at least 2 bases from its neighbours and not at a contig end has the window that starts one
// base in front of it and the one that ends one base behind it as its anchors; when those are at most `max` apart and hold bases only
// it is a site.  One hypo_gpu_kset_query_walks call (kset_kernel.hip) walks the set as a de Bruijn graph from the left anchor to the
// right one, allowing the stretch to grow or shrink by `slack` bases, and a site with exactly one walk gets that walk's text.  Every
// window of the new stretch is an anchor or a k-mer of the walk, and nothing outside it moves, so a contig's missing k-mers drop by
// exactly the bridged intervals' counts.
// --kmer-bridge-vote <ratio> (DESIGN.md "k-mer bridge vote"): the sites that call leaves AMBIGUOUS are asked again through
// hypo_gpu_kset_query_walk_sets, which reports up to 4 walks with the least read count along each.  When that search ends AMBIGUOUS
// too and the best support is at least `ratio` times the second best, the best walk is the site's walk and the site is bridged as a
// unique one is; close supports, more than 4 walks and a search over budget leave it alone.
#pragma once
#include <cstdint>
#include <ostream>
#include <string>
#include <vector>
#include "KmerFix.hpp"
#include "ReadKmerSet.hpp"

namespace hypo {

class KmerBridge {
public:
    static constexpr uint32_t kBudget = 4096;                // visits a site's search may make
    static constexpr uint32_t kMaxDefault = 64, kMaxLo = 2, kMaxHi = 192;          // --kmer-bridge-max
    static constexpr uint32_t kSlackDefault = 8, kSlackLo = 0, kSlackHi = 64;      // --kmer-bridge-slack (kMaxHi + kSlackHi = HYPO_KSET_MAX_WALK)
    static constexpr uint32_t kVoteLo = 2, kVoteHi = 255;   // --kmer-bridge-vote
    struct Stats { uint64_t intervals = 0, sites = 0, bridged = 0, bases_out = 0, bases_in = 0, ambiguous = 0, over_budget = 0, removed = 0; };
    struct VoteStats { uint64_t asked = 0, chosen = 0, close = 0, many = 0, over_budget = 0; };     // asked = the sum of the others
    using Emit = KmerFix::Emit;                               // what a contig's turn hands on: the draft it came with and the new text

    explicit KmerBridge(const ReadKmerSet& set) : _set(set) {}        // the set that is asked (its track query must be bound), and its k
    // binds hypo_gpu_kset_query_walks by name (false: the device library does not provide it)
    bool bind();
    // --kmer-bridge-vote: binds hypo_gpu_kset_query_walk_sets by name (false: the device library does not provide it); the set must count
    bool bind_vote();
    void configure_vote(uint32_t ratio) { _ratio = ratio; }
    uint32_t vote_ratio() const { return _ratio; }           // 0: no vote
    const VoteStats& vote_stats() const { return _vstats; }
    void configure(uint32_t max_dist, uint32_t slack) { _max = max_dist; _slack = slack; }
    uint32_t k() const { return _set.k(); }
    uint32_t max_dist() const { return _max; }
    uint32_t slack() const { return _slack; }
    // as KmerFix::push / flush: at most ReadKmerSet::kTextPerCall of text a call, `emit` gets every contig in the order they were pushed
    int push(uint32_t contig, const std::string& name, std::string draft, std::string text, const Emit& emit);
    int flush(const Emit& emit);
    const Stats& stats() const { return _stats; }
    // "#contig pos ref alt missing_kmers steps", one line per bridge, contigs in the order they were pushed, pos ascending (0-based, in
    // the text before this pass); under the vote two more columns, "walks support": 1 and "." for a unique bridge, the walks found and
    // best/second for a chosen one (whose steps are the second search's)
    void write(std::ostream& os) const;
private:
    const ReadKmerSet& _set;
    struct Pending { uint32_t contig = 0; std::string name, draft; uint64_t off = 0, len = 0; };
    int (*_walks)(const char*, uint64_t, const uint64_t*, const uint64_t*, const uint32_t*, const uint32_t*, uint32_t, uint32_t, uint32_t*, uint32_t*, uint32_t*,
                  uint8_t*) = nullptr;
    int (*_walk_sets)(const char*, uint64_t, const uint64_t*, const uint64_t*, const uint32_t*, const uint32_t*, uint32_t, uint32_t, uint32_t*, uint32_t*, uint32_t*,
                      uint32_t*, uint32_t*, uint8_t*) = nullptr;
    uint32_t _ratio = 0;
    VoteStats _vstats;
    uint32_t _max = kMaxDefault, _slack = kSlackDefault;
    Stats _stats;
    std::string _text;                                       // the texts of the pending contigs, back to back
    std::vector<Pending> _pending;
    std::string _lines;                                      // the TSV's lines so far
};

}  // namespace hypo
