// CnReport.hpp — hypo --qv-cn: where the copy number of the text that is written disagrees with the reads (DESIGN.md "k-mer copy
// number").  A collapsed repeat or a falsely duplicated stretch loses no k-mer, so --qv and --qv-bed do not see it; what gives it
// away is how often the reads contain the k-mers of a stretch against how often the whole text does.  The set counts
// (ReadKmerSet::enable_counts), one of its text planes holds the copy bytes of the final text, and per bin of every contig
// hypo_gpu_kset_query_depth compares the two bytes of every window (ReadKmerSet::query_depth).
// A repeat's second copy may lie in the last contig, so every contig's final text (after guard, fixes and bridges) is kept, one byte
// a base, until the last batch is written; run() then marks the text (unless --qv-spectra has done so: its polished plane is used)
// and makes the depth pass, while the set lives.
#pragma once
#include <cstdint>
#include <ostream>
#include <string>
#include <vector>
#include "ReadKmerSet.hpp"

namespace hypo {

class CnReport {
public:
    explicit CnReport(const ReadKmerSet& set) : _set(set) {}
    // binds hypo_gpu_kset_mark by name (false: the device library lacks it); the depth query is the set's (ReadKmerSet::bind_depth)
    bool bind();
    // bin: window starts per line; unit: reads per copy, 0 = the peak of the read histogram; plane: the text plane to compare
    // against, which run() marks itself when own_mark is set
    void configure(uint32_t bin, uint32_t unit, uint32_t plane, bool own_mark) { _bin = bin; _unit = unit; _given = unit != 0; _plane = plane; _own_mark = own_mark; }
    void push(size_t contig, const std::string& polished);  // one contig's final text
    // behind the last contig, while the set lives.  HYPO_OK, the C-ABI's error (`what` names the entry point), or E_NO_PEAK: no unit
    // was given and the read histogram has no peak at or above its valley
    static constexpr int E_NO_PEAK = 1;
    int run(const char*& what);
    // "#contig start end windows missing rated over under median_count call", contigs in draft order
    void write(std::ostream& os, const std::vector<std::string>& names) const;
    uint32_t k() const { return _set.k(); }
    uint32_t bin() const { return _bin; }
    uint32_t unit() const { return _unit; }
    bool unit_given() const { return _given; }
    struct Sums { uint64_t bins = 0, collapsed = 0, collapsed_bases = 0, duplicated = 0, duplicated_bases = 0; };
    Sums sums() const;
private:
    // 1 collapsed, 2 duplicated, 0 neither, of bin b
    int call_of(size_t b) const { return 2 * (uint64_t)_d.over[b] > _d.rated[b] ? 1 : 2 * (uint64_t)_d.under[b] > _d.rated[b] ? 2 : 0; }
    template <class F> void each_bin(F f) const;             // f(contig, start, end, bin index), contigs in draft order
    const ReadKmerSet& _set;
    int (*_mark)(uint32_t, const char*, const uint64_t*, uint32_t, uint64_t*, uint64_t*) = nullptr;
    uint32_t _bin = 1024, _unit = 0, _plane = 0;
    bool _given = false, _own_mark = true;
    std::string _text;                                       // the final texts, back to back in the order they were written
    std::vector<uint64_t> _off{0};
    std::vector<size_t> _who;                                // contig of every text in _text
    ReadKmerSet::Depth _d;
};

}  // namespace hypo
