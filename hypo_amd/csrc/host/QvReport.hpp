// QvReport.hpp — hypo --qv: the reference-free k-mer QV of every draft contig and of its polished text (DESIGN.md "k-mer QV").
// The canonical k-mers of the short reads are kept as an exact set on device context 0 (hypo_gpu_kset_*, kset_kernel.hip), filled
// by the parse pass of stage 0; the writer thread asks it, per contig batch, how many k-mers of the drafts and of the polished
// texts it lacks.  QV = -10 log10(1 - (1 - missing / total)^(1 / k)) (Merqury's definition: a k-mer seen once is present).
#pragma once
#include <cstdint>
#include <ostream>
#include <string>
#include <vector>
#include "SolidBuild.hpp"

namespace hypo {

// "%.2f" of the QV; "inf" when nothing is missing, "NA" when there is no window
std::string qv_text(uint64_t missing, uint64_t total, uint32_t k);

class QvReport {
public:
    // binds hypo_gpu_kset_* by name: only runs with --qv need them (false: the device library does not provide them)
    bool bind();
    // --qv-bed: binds hypo_gpu_kset_query_track as well (false: the library does not provide it).  From then on flush() asks with it
    // instead of hypo_gpu_kset_query, and keeps the intervals of every polished text.
    bool bind_track();
    // the set on the calling thread's context; max_bytes 0 = the library's default cap
    int begin(uint32_t k, uint64_t expected_distinct, uint64_t max_bytes, size_t n_contigs);
    // --qv-min-count: binds hypo_gpu_kset_counts_enable, _spectrum and _min_count by name (false: the library lacks one).  The
    // set counts (enable_counts right after begin, unless --qv-spectra has enabled its counts already), and after the reads
    // set_min_count reads the histogram of the read counts, takes t = `given` or, for 0, its valley, and from then on every query of
    // the set, the guard's included, is answered against the k-mers seen at least t times (DESIGN.md "k-mer min count").
    bool bind_min_count();
    int enable_counts();
    int set_min_count(uint32_t given);
    uint32_t min_count() const { return _min_count; }
    uint64_t n_reliable() const { return _n_reliable; }      // distinct read k-mers seen at least min_count() times
    ReadSink sink();
    int read_size();                                         // after the reads: fetches the number of distinct k-mers
    uint64_t n_distinct() const { return _n_distinct; }
    uint32_t k() const { return _k; }
    // one contig's two texts; they are queried (one call on the calling thread's context) when flush() is called or enough text has
    // gathered.  HYPO_OK or the C-ABI's error.
    int push(size_t contig, const std::string& draft, const std::string& polished);
    int flush();
    void end();                                              // frees the set (safe to call twice)
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
    int (*_begin)(uint32_t, uint64_t, uint64_t) = nullptr;
    int (*_add)(const char*, uint64_t) = nullptr;
    int (*_size)(uint64_t*, uint64_t*) = nullptr;
    int (*_query)(const char*, const uint64_t*, uint32_t, uint64_t*, uint64_t*) = nullptr;
    int (*_end)(void) = nullptr;
    int (*_track)(const char*, const uint64_t*, uint32_t, const uint8_t*, uint64_t*, uint64_t*, uint64_t*, uint64_t*, uint64_t*, uint64_t*, uint64_t) = nullptr;
    struct Interval { uint64_t start, end, missing; };
    std::vector<std::vector<Interval>> _intervals;           // per contig, of its polished text
    int (*_counts_enable)(uint32_t) = nullptr;
    int (*_spectrum)(uint32_t, uint64_t*) = nullptr;
    int (*_set_min_count)(uint32_t) = nullptr;
    uint32_t _min_count = 1;
    uint64_t _n_reliable = 0;
    bool _open = false;
    uint32_t _k = 0;
    uint64_t _n_distinct = 0;
    std::vector<Row> _rows;
    std::string _text;                                       // the texts waiting for a query, back to back
    std::vector<uint64_t> _off;
    std::vector<size_t> _who;                                // contig of every pair of texts in _text
};

}  // namespace hypo
