// QvReport.hpp — hypo --qv: the reference-free k-mer QV of every draft contig and of its polished text (DESIGN.md "k-mer QV").
// The canonical k-mers of the short reads are an exact set on device context 0 (ReadKmerSet); the writer thread asks it, per contig
// batch, how many k-mers of the drafts and of the polished texts it lacks.  QV = -10 log10(1 - (1 - missing / total)^(1 / k))
// (Merqury's definition: a k-mer seen once is present).  hypo --qv-bed (DESIGN.md "k-mer QV track"): the same question through
// the set's track query, which also says where the missing k-mers of the polished texts are.
#pragma once
#include <cstdint>
#include <ostream>
#include <string>
#include <vector>
#include "ReadKmerSet.hpp"

namespace hypo {

// "%.2f" of the QV; "inf" when nothing is missing, "NA" when there is no window
std::string qv_text(uint64_t missing, uint64_t total, uint32_t k);

class QvReport {
public:
    explicit QvReport(const ReadKmerSet& set) : _set(set) {}
    // binds hypo_gpu_kset_query by name: only runs with --qv need it (false: the device library does not provide it)
    bool bind();
    // --qv-bed: from here on flush() asks with the set's track query (ReadKmerSet::bind_track) instead of hypo_gpu_kset_query, and
    // keeps the intervals of every polished text
    void keep_track() { _keep_track = true; }
    // one contig's two texts; they are queried (one call on the calling thread's context) when flush() is called or enough text has
    // gathered.  HYPO_OK or the C-ABI's error.
    int push(size_t contig, const std::string& draft, const std::string& polished);
    int flush();
    // the table: one row per contig in draft order, then the sums as contig "*"
    void write(std::ostream& os, const std::vector<std::string>& names) const;
    std::string draft_qv() const, polished_qv() const;       // of the sums
    // the track: "#contig start end missing_kmers", one line per interval of a polished text, contigs in draft order
    void write_track(std::ostream& os, const std::vector<std::string>& names) const;
    struct TrackSums { uint64_t intervals = 0, bases = 0, missing = 0; };
    TrackSums track_sums() const;
private:
    struct Row { uint64_t dm = 0, dt = 0, pm = 0, pt = 0; };
    Row sums() const;
    const ReadKmerSet& _set;
    int (*_query)(const char*, const uint64_t*, uint32_t, uint64_t*, uint64_t*) = nullptr;
    bool _keep_track = false;
    struct Interval { uint64_t start, end, missing; };
    std::vector<std::vector<Interval>> _intervals;           // per contig, of its polished text
    std::vector<Row> _rows;
    std::string _text;                                       // the texts waiting for a query, back to back
    std::vector<uint64_t> _off{0};
    std::vector<size_t> _who;                                // contig of every pair of texts in _text
};

}  // namespace hypo
