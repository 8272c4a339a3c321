// QvReport.cpp — see QvReport.hpp.
#include "QvReport.hpp"
#include <dlfcn.h>
#include <cmath>
#include <cstdio>

namespace hypo {

std::string qv_text(uint64_t missing, uint64_t total, uint32_t k) {
    if (!total) return "NA";
    if (!missing) return "inf";
    const double err = 1.0 - std::pow(1.0 - (double)missing / (double)total, 1.0 / (double)k);
    char b[64];
    std::snprintf(b, sizeof b, "%.2f", -10.0 * std::log10(err) + 0.0);          // (+ 0.0: every k-mer missing prints 0.00, not -0.00)
    return b;
}

bool QvReport::bind() {
    _query = (decltype(_query))dlsym(RTLD_DEFAULT, "hypo_gpu_kset_query");
    return _query != nullptr;
}

int QvReport::push(size_t contig, const std::string& draft, const std::string& polished) {
    if (_rows.size() <= contig) _rows.resize(contig + 1);
    _text += draft; _off.push_back(_text.size());
    _text += polished; _off.push_back(_text.size());
    _who.push_back(contig);
    return _text.size() >= ReadKmerSet::kTextPerCall ? flush() : HYPO_OK;
}

int QvReport::flush() {
    if (_who.empty()) return HYPO_OK;
    const uint32_t n = (uint32_t)(_off.size() - 1);
    ReadKmerSet::Track t;
    if (_keep_track) {
        // intervals of the polished texts only (the odd sequences)
        std::vector<uint8_t> want(n);
        for (uint32_t s = 0; s < n; ++s) want[s] = s & 1;
        const int rc = _set.query_track(_text, _off, want.data(), t);
        if (rc != HYPO_OK) return rc;
        if (_intervals.size() < _rows.size()) _intervals.resize(_rows.size());
        for (size_t i = 0; i < _who.size(); ++i) {
            std::vector<Interval>& iv = _intervals[_who[i]];
            iv.clear();
            for (uint64_t j = t.iv_off[2 * i + 1]; j < t.iv_off[2 * i + 2]; ++j) iv.push_back(Interval{t.start[j], t.end[j], t.count[j]});
        }
    } else {
        t.total.resize(n); t.missing.resize(n);
        const int rc = _query(_text.data(), _off.data(), n, t.total.data(), t.missing.data());
        if (rc != HYPO_OK) return rc;
    }
    for (size_t i = 0; i < _who.size(); ++i) {
        Row& r = _rows[_who[i]];
        r.dt = t.total[2 * i]; r.dm = t.missing[2 * i]; r.pt = t.total[2 * i + 1]; r.pm = t.missing[2 * i + 1];
    }
    _text.clear(); _off.assign(1, 0); _who.clear();
    return HYPO_OK;
}

QvReport::Row QvReport::sums() const {
    Row s;
    for (const Row& r : _rows) { s.dm += r.dm; s.dt += r.dt; s.pm += r.pm; s.pt += r.pt; }
    return s;
}
std::string QvReport::draft_qv() const { const Row s = sums(); return qv_text(s.dm, s.dt, _set.k()); }
std::string QvReport::polished_qv() const { const Row s = sums(); return qv_text(s.pm, s.pt, _set.k()); }

void QvReport::write(std::ostream& os, const std::vector<std::string>& names) const {
    os << "#contig\tdraft_missing\tdraft_total\tdraft_qv\tpolished_missing\tpolished_total\tpolished_qv\n";
    const uint32_t k = _set.k();
    auto row = [&](const std::string& name, const Row& r) {
        os << name << '\t' << r.dm << '\t' << r.dt << '\t' << qv_text(r.dm, r.dt, k) << '\t' << r.pm << '\t' << r.pt << '\t' << qv_text(r.pm, r.pt, k) << '\n';
    };
    for (size_t i = 0; i < names.size(); ++i) row(names[i], i < _rows.size() ? _rows[i] : Row());
    row("*", sums());
}

void QvReport::write_track(std::ostream& os, const std::vector<std::string>& names) const {
    os << "#contig\tstart\tend\tmissing_kmers\n";
    for (size_t i = 0; i < names.size() && i < _intervals.size(); ++i)
        for (const Interval& iv : _intervals[i]) os << names[i] << '\t' << iv.start << '\t' << iv.end << '\t' << iv.missing << '\n';
}

QvReport::TrackSums QvReport::track_sums() const {
    TrackSums s;
    for (const auto& ivs : _intervals)
        for (const Interval& iv : ivs) { ++s.intervals; s.bases += iv.end - iv.start; s.missing += iv.missing; }
    return s;
}

}  // namespace hypo
