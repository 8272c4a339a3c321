// CnReport.cpp — see CnReport.hpp.
#include "CnReport.hpp"
#include <dlfcn.h>

namespace hypo {

bool CnReport::bind() {
    _mark = (decltype(_mark))dlsym(RTLD_DEFAULT, "hypo_gpu_kset_mark");
    return _mark != nullptr;
}

void CnReport::push(size_t contig, const std::string& polished) {
    _text += polished;
    _off.push_back(_text.size());
    _who.push_back(contig);
}

int CnReport::run(const char*& what) {
    const size_t n = _who.size();
    // the whole text is marked before the first bin is asked: calls of whole contigs, as far as they fit
    what = "hypo_gpu_kset_mark";
    for (size_t s = 0; _own_mark && s < n;) {
        size_t e = s + 1;
        while (e < n && _off[e + 1] - _off[s] <= ReadKmerSet::kTextPerCall) ++e;
        const int rc = _mark(_plane, _text.data(), _off.data() + s, (uint32_t)(e - s), nullptr, nullptr);
        if (rc != HYPO_OK) return rc;
        s = e;
    }
    if (!_given) {
        what = "hypo_gpu_kset_spectrum";
        std::vector<uint64_t> hist;
        const int rc = _set.spectrum(_plane, hist);
        if (rc != HYPO_OK) return rc;
        uint64_t h[ReadKmerSet::kRows];
        for (uint32_t c = 0; c < ReadKmerSet::kRows; ++c) { h[c] = 0; for (uint32_t j = 0; j < ReadKmerSet::kCols; ++j) h[c] += hist[(size_t)c * ReadKmerSet::kCols + j]; }
        _unit = ReadKmerSet::peak(h);
        if (!_unit) return E_NO_PEAK;
    }
    what = "hypo_gpu_kset_query_depth";
    const int rc = _set.query_depth(_text, _off, _bin, _plane, _unit, _d);
    std::string().swap(_text);
    return rc;
}

template <class F> void CnReport::each_bin(F f) const {
    std::vector<uint64_t> first(_who.size() + 1, 0);         // the first bin of every text
    size_t n_contigs = 0;
    for (size_t i = 0; i < _who.size(); ++i) {
        first[i + 1] = first[i] + (_off[i + 1] - _off[i] + _bin - 1) / _bin;
        if (_who[i] >= n_contigs) n_contigs = _who[i] + 1;
    }
    std::vector<size_t> text_of(n_contigs, (size_t)-1);
    for (size_t i = 0; i < _who.size(); ++i) text_of[_who[i]] = i;
    for (size_t c = 0; c < n_contigs; ++c) {
        const size_t i = text_of[c];
        if (i == (size_t)-1) continue;
        const uint64_t len = _off[i + 1] - _off[i];
        for (uint64_t b = first[i]; b < first[i + 1] && b < _d.windows.size(); ++b) {
            const uint64_t start = (b - first[i]) * _bin;
            f(c, start, start + _bin < len ? start + _bin : len, (size_t)b);
        }
    }
}

void CnReport::write(std::ostream& os, const std::vector<std::string>& names) const {
    os << "##hypo-qv-cn\tk=" << _set.k() << "\tbin=" << _bin << "\tunit=" << _unit << '\t' << (_given ? "given" : "peak") << "\tmin_count=" << _set.min_count() << '\n';
    os << "#contig\tstart\tend\twindows\tmissing\trated\tover\tunder\tmedian_count\tcall\n";
    static const char* const call[3] = {".", "collapsed", "duplicated"};
    each_bin([&](size_t c, uint64_t start, uint64_t end, size_t b) {
        os << names[c] << '\t' << start << '\t' << end << '\t' << _d.windows[b] << '\t' << _d.missing[b] << '\t' << _d.rated[b] << '\t' << _d.over[b] << '\t'
           << _d.under[b] << '\t' << (unsigned)_d.median[b] << '\t' << call[call_of(b)] << '\n';
    });
}

CnReport::Sums CnReport::sums() const {
    Sums s;
    each_bin([&](size_t, uint64_t start, uint64_t end, size_t b) {
        ++s.bins;
        const int what = call_of(b);
        if (what == 1) { ++s.collapsed; s.collapsed_bases += end - start; }
        if (what == 2) { ++s.duplicated; s.duplicated_bases += end - start; }
    });
    return s;
}

}  // namespace hypo
