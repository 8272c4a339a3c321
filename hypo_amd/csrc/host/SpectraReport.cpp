// SpectraReport.cpp — see SpectraReport.hpp.
#include "SpectraReport.hpp"
#include <dlfcn.h>
#include <cstdio>

namespace hypo {

bool SpectraReport::bind() {
    _mark = (decltype(_mark))dlsym(RTLD_DEFAULT, "hypo_gpu_kset_mark");
    return _mark != nullptr;
}

int SpectraReport::push(const std::string& draft, const std::string& polished) {
    _text[DRAFT] += draft; _off[DRAFT].push_back(_text[DRAFT].size());
    _text[POLISHED] += polished; _off[POLISHED].push_back(_text[POLISHED].size());
    return _text[DRAFT].size() + _text[POLISHED].size() >= ReadKmerSet::kTextPerCall ? flush() : HYPO_OK;
}

int SpectraReport::flush() {
    for (int t = 0; t < N_TEXTS; ++t) {
        if (_off[t].size() < 2) continue;
        uint64_t unmarked = 0;
        const int rc = _mark((uint32_t)t, _text[t].data(), _off[t].data(), (uint32_t)(_off[t].size() - 1), nullptr, &unmarked);
        if (rc != HYPO_OK) return rc;
        _asm_only[t] += unmarked;
        _text[t].clear(); _off[t].assign(1, 0);
    }
    return HYPO_OK;
}

int SpectraReport::fetch(uint32_t reliable_min) {
    for (int t = 0; t < N_TEXTS; ++t) {
        std::string().swap(_text[t]);
        const int rc = _set.spectrum((uint32_t)t, _hist[t]);
        if (rc != HYPO_OK) return rc;
    }
    _given = reliable_min != 0;
    _t = reliable_min;
    if (!_given) {
        uint64_t h[kRows];
        for (uint32_t c = 0; c < kRows; ++c) { h[c] = 0; for (uint32_t j = 0; j < kCols; ++j) h[c] += at(DRAFT, c, j); }
        _t = ReadKmerSet::valley(h);
    }
    return HYPO_OK;
}

void SpectraReport::sums(Text t, uint64_t& reliable, uint64_t& found) const {
    reliable = found = 0;
    for (uint32_t c = _t; c < kRows; ++c)
        for (uint32_t j = 0; j < kCols; ++j) { reliable += at(t, c, j); if (j) found += at(t, c, j); }
}

std::string SpectraReport::completeness(Text t) const {
    uint64_t reliable, found;
    sums(t, reliable, found);
    if (!reliable) return "NA";
    char b[64];
    std::snprintf(b, sizeof b, "%.6f", (double)found / (double)reliable);
    return b;
}

void SpectraReport::write(std::ostream& os) const {
    os << "##hypo-qv-spectra\tk=" << _set.k() << "\treads_distinct=" << _set.n_distinct() << "\treliable_min=" << _t << '\t' << (_given ? "given" : "valley") << '\n';
    os << "#text\treliable\tfound\tcompleteness\tasm_only_windows\n";
    static const char* const name[N_TEXTS] = {"draft", "polished"};
    for (int t = 0; t < N_TEXTS; ++t) {
        uint64_t reliable, found;
        sums((Text)t, reliable, found);
        os << name[t] << '\t' << reliable << '\t' << found << '\t' << completeness((Text)t) << '\t' << _asm_only[t] << '\n';
    }
    os << "#multiplicity";
    for (int t = 0; t < N_TEXTS; ++t)
        for (uint32_t j = 0; j < kCols; ++j) os << '\t' << name[t] << "_cn" << j << (j + 1 == kCols ? "+" : "");
    os << '\n';
    for (uint32_t c = 1; c < kRows; ++c) {
        os << c;
        for (int t = 0; t < N_TEXTS; ++t)
            for (uint32_t j = 0; j < kCols; ++j) os << '\t' << at((Text)t, c, j);
        os << '\n';
    }
}

}  // namespace hypo
