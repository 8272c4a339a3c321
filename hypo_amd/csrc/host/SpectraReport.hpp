// SpectraReport.hpp — hypo --qv-spectra: how often the reads contain every k-mer, how often the draft and the polished text
// contain it, and from the two the copy-number spectrum and the k-mer completeness of both texts (DESIGN.md "k-mer spectra";
// Merqury's spectra-cn and completeness).  The k-mer set of the reads counts (ReadKmerSet::enable_counts(N_TEXTS), right after the
// set exists), the writer thread marks every contig's two texts where QvReport queries them (hypo_gpu_kset_mark, text 0 = draft,
// text 1 = polished, on context 0), and behind the last contig the two spectra come back (ReadKmerSet::spectrum).
#pragma once
#include <cstdint>
#include <ostream>
#include <string>
#include <vector>
#include "ReadKmerSet.hpp"

namespace hypo {

class SpectraReport {
public:
    enum Text { DRAFT = 0, POLISHED = 1, N_TEXTS = 2 };
    explicit SpectraReport(const ReadKmerSet& set) : _set(set) {}
    // binds hypo_gpu_kset_mark by name: only runs with --qv-spectra need it (false: the device library lacks it)
    bool bind();
    // one contig's two texts; they are marked (one call per text) when flush() is called or enough text has gathered
    int push(const std::string& draft, const std::string& polished);
    int flush();
    // behind the last contig, while the set lives: the two spectra, and the threshold (reliable_min 0: the valley of the read histogram)
    int fetch(uint32_t reliable_min);
    void write(std::ostream& os) const;
    uint32_t k() const { return _set.k(); }
    uint32_t threshold() const { return _t; }
    std::string completeness(Text t) const;                  // "%.6f" of found / reliable, "NA" without a reliable k-mer
    uint64_t asm_only(Text t) const { return _asm_only[t]; }
private:
    static constexpr uint32_t kRows = ReadKmerSet::kRows, kCols = ReadKmerSet::kCols;
    uint64_t at(Text t, uint32_t c, uint32_t j) const { return _hist[t][(size_t)c * kCols + j]; }
    void sums(Text t, uint64_t& reliable, uint64_t& found) const;
    const ReadKmerSet& _set;
    int (*_mark)(uint32_t, const char*, const uint64_t*, uint32_t, uint64_t*, uint64_t*) = nullptr;
    std::string _text[N_TEXTS];                              // the texts waiting for their mark call, back to back
    std::vector<uint64_t> _off[N_TEXTS] = {{0}, {0}};
    uint64_t _asm_only[N_TEXTS] = {0, 0};                    // windows whose k-mer no read contains
    std::vector<uint64_t> _hist[N_TEXTS];
    uint32_t _t = 0;
    bool _given = false;
};

}  // namespace hypo
