// KmerGuard.hpp — hypo --kmer-guard: only the edits the k-mers of the short reads support reach the output (DESIGN.md "k-mer
// guard").  The VCF records of a contig (EditVcf) that lie closer than k - 1 unchanged draft bases form a cluster; no length-k window
// touches the edits of two clusters, so each is judged alone: its draft text and its polished text, each with the k - 1 bases on
// either side, are two spans of one hypo_gpu_kset_query_spans call on context 0 (kset_kernel.hip), and a cluster whose polished span
// lacks more k-mers of the reads' set (ReadKmerSet) than its draft span is rejected with all its records.  The FASTA record is
// the draft with the accepted records applied.
// hypo --guard-records (DESIGN.md "k-mer guard by record"): a cluster of 2 .. N records is one site of a
// hypo_gpu_kset_query_variants call, its records the site's edits, and of all subsets of them the one the call names best is
// kept; a larger cluster is a site with ONE edit, its draft span replaced by its polished span, which is the decision above.
// Only the drafts and the ALT strings go to the device.
#pragma once
#include <cstdint>
#include <functional>
#include <memory>
#include <string>
#include <vector>
#include "Contig.hpp"
#include "EditVcf.hpp"
#include "ReadKmerSet.hpp"

namespace hypo {

class KmerGuard {
public:
    // rejected_clusters: rejected with all their records; partial_clusters: with some (by record only); by_size[n]: clusters of n
    // records, n = 1 .. N, and [0] those of more (by record only)
    struct Stats { uint64_t clusters = 0, records = 0, rejected_clusters = 0, rejected_records = 0, partial_clusters = 0; uint64_t by_size[13] = {}; };
    // One contig's clusters: records [first[c], first[c + 1]) of the contig form cluster c; its draft span [b, e) and polished span
    // [qb, qe) without the flanks.
    struct Cluster { size_t r0 = 0, r1 = 0; uint64_t b = 0, e = 0, qb = 0, qe = 0; };
    // what a contig's turn hands to the writer: the draft, the guarded text, the records and which of them were rejected
    using Emit = std::function<int(uint32_t contig, const std::string& draft, const std::string& text, const VcfContigRecords& recs, const std::vector<uint8_t>& rejected)>;

    explicit KmerGuard(const ReadKmerSet& set) : _set(set) {}         // the set the spans are put to; the clusters are cut with its k
    // binds hypo_gpu_kset_query_spans by name (false: the device library does not provide it)
    bool bind();
    // --guard-records: binds hypo_gpu_kset_query_variants by name (false: the device library does not provide it); clusters of up
    // to max_records (2..12) records are decided record by record from here on
    bool bind_variants(uint32_t max_records);
    bool by_record() const { return _variants != nullptr; }
    uint32_t max_records() const { return _max_records; }
    // the clusters of one contig's records (the rule above); polished spans follow from the records' length changes
    static void clusters_of(const std::vector<VcfRec>& recs, uint32_t k, std::vector<Cluster>& out);
    // the draft with the records that are not rejected applied
    static std::string apply(const std::string& draft, const std::vector<VcfRec>& recs, const std::vector<uint8_t>& rejected);
    // Contigs [c0, c1) of a batch whose edit scripts are in `eb`: records, clusters, the spans calls on the calling thread's context
    // (at most ReadKmerSet::kTextPerCall of text a call; a larger contig gets a call of its own), decisions, and `emit` for every contig
    // in order.  HYPO_OK, the C-ABI's error, or what emit answered.
    int run_batch(const std::vector<std::unique_ptr<Contig>>& contigs, uint32_t c0, uint32_t c1, const EditBatchResult& eb, VcfStats& vst, const Emit& emit);
    const Stats& stats() const { return _stats; }
    uint32_t k() const { return _set.k(); }
private:
    struct Pending { uint32_t contig = 0; uint64_t d_off = 0, d_len = 0, p_off = 0, p_len = 0; VcfContigRecords recs; std::vector<Cluster> clusters; size_t span0 = 0; };
    int flush(const Emit& emit);
    int flush_by_record(const Emit& emit);
    const ReadKmerSet& _set;
    int (*_variants)(const char*, uint64_t, const char*, uint64_t, const uint64_t*, const uint64_t*, const uint32_t*, uint32_t, const uint64_t*, const uint64_t*,
                     const uint64_t*, const uint32_t*, uint32_t*, uint64_t*, uint64_t*, uint64_t*, uint64_t*) = nullptr;
    uint32_t _max_records = 8;
    // by record: the ALT strings (and the polished spans of the clusters decided whole) back to back, one site per cluster
    // ([_lo, _hi) as above, one entry a cluster), the sites' edits, and the polished texts (kept on the host for emit)
    std::string _alts;
    std::vector<uint32_t> _edit_off, _al;
    std::vector<uint64_t> _eb, _ee, _ao;
    std::vector<std::string> _polished;
    uint64_t _n_variants = 0;
    int (*_spans)(const char*, uint64_t, const uint64_t*, const uint64_t*, uint32_t, uint64_t*, uint64_t*) = nullptr;
    Stats _stats;
    std::string _text;                                       // D and P of the pending contigs, back to back
    std::vector<uint64_t> _lo, _hi;                          // two spans per cluster: draft, polished
    std::vector<Pending> _pending;
};

}  // namespace hypo
