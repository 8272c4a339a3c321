// QvReport.cpp — see QvReport.hpp.
#include "QvReport.hpp"
#include "SpectraReport.hpp"
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
    _begin = (decltype(_begin))dlsym(RTLD_DEFAULT, "hypo_gpu_kset_begin");
    _add = (decltype(_add))dlsym(RTLD_DEFAULT, "hypo_gpu_kset_add");
    _size = (decltype(_size))dlsym(RTLD_DEFAULT, "hypo_gpu_kset_size");
    _query = (decltype(_query))dlsym(RTLD_DEFAULT, "hypo_gpu_kset_query");
    _end = (decltype(_end))dlsym(RTLD_DEFAULT, "hypo_gpu_kset_end");
    return _begin && _add && _size && _query && _end;
}

bool QvReport::bind_track() {
    _track = (decltype(_track))dlsym(RTLD_DEFAULT, "hypo_gpu_kset_query_track");
    return _track != nullptr;
}

bool QvReport::bind_min_count() {
    _counts_enable = (decltype(_counts_enable))dlsym(RTLD_DEFAULT, "hypo_gpu_kset_counts_enable");
    _spectrum = (decltype(_spectrum))dlsym(RTLD_DEFAULT, "hypo_gpu_kset_spectrum");
    _set_min_count = (decltype(_set_min_count))dlsym(RTLD_DEFAULT, "hypo_gpu_kset_min_count");
    return _counts_enable && _spectrum && _set_min_count;
}

int QvReport::enable_counts() { return _counts_enable(1); }

int QvReport::set_min_count(uint32_t given) {
    // no text has been marked yet: every key of the set is in column 0 of its count's row
    std::vector<uint64_t> hist((size_t)SpectraReport::kRows * SpectraReport::kCols);
    int rc = _spectrum(0, hist.data());
    if (rc != HYPO_OK) return rc;
    uint64_t h[SpectraReport::kRows];
    for (uint32_t c = 0; c < SpectraReport::kRows; ++c) { h[c] = 0; for (uint32_t j = 0; j < SpectraReport::kCols; ++j) h[c] += hist[(size_t)c * SpectraReport::kCols + j]; }
    const uint32_t t = given ? given : SpectraReport::valley(h);
    if ((rc = _set_min_count(t)) != HYPO_OK) return rc;
    _min_count = t; _n_reliable = 0;
    for (uint32_t c = t; c < SpectraReport::kRows; ++c) _n_reliable += h[c];
    return HYPO_OK;
}

int QvReport::begin(uint32_t k, uint64_t expected_distinct, uint64_t max_bytes, size_t n_contigs) {
    const int rc = _begin(k, expected_distinct, max_bytes);
    if (rc != HYPO_OK) return rc;
    _open = true; _k = k;
    _rows.assign(n_contigs, Row());
    _off.assign(1, 0);
    return HYPO_OK;
}

ReadSink QvReport::sink() {
    ReadSink s;
    s.k = _k;
    s.add = [this](const char* p, uint64_t n) { return _add(p, n); };
    return s;
}

int QvReport::read_size() { return _size(&_n_distinct, nullptr); }

int QvReport::push(size_t contig, const std::string& draft, const std::string& polished) {
    constexpr size_t kFlushAt = (size_t)512 << 20;           // text per query call (a batch of small contigs: one call)
    if (_rows.size() <= contig) _rows.resize(contig + 1);
    _text += draft; _off.push_back(_text.size());
    _text += polished; _off.push_back(_text.size());
    _who.push_back(contig);
    return _text.size() >= kFlushAt ? flush() : HYPO_OK;
}

int QvReport::flush() {
    if (_who.empty()) return HYPO_OK;
    const uint32_t n = (uint32_t)(_off.size() - 1);
    std::vector<uint64_t> total(n), missing(n);
    int rc;
    if (_track) {
        // intervals of the polished texts only (the odd sequences); a call that finds more than there is room for says how many
        std::vector<uint8_t> want(n);
        for (uint32_t s = 0; s < n; ++s) want[s] = s & 1;
        const size_t room = 1024 + _text.size() / 1024;         // (a retry asks the set everything again: rare at one interval per kbp)
        std::vector<uint64_t> iv_off(n + 1), start(room), end(room), count(room);
        rc = _track(_text.data(), _off.data(), n, want.data(), total.data(), missing.data(), iv_off.data(), start.data(), end.data(), count.data(), start.size());
        if (rc == HYPO_E_WORKSPACE) {
            start.resize(iv_off[n]); end.resize(iv_off[n]); count.resize(iv_off[n]);
            rc = _track(_text.data(), _off.data(), n, want.data(), total.data(), missing.data(), iv_off.data(), start.data(), end.data(), count.data(), start.size());
        }
        if (rc != HYPO_OK) return rc;
        if (_intervals.size() < _rows.size()) _intervals.resize(_rows.size());
        for (size_t i = 0; i < _who.size(); ++i) {
            std::vector<Interval>& iv = _intervals[_who[i]];
            iv.clear();
            for (uint64_t j = iv_off[2 * i + 1]; j < iv_off[2 * i + 2]; ++j) iv.push_back(Interval{start[j], end[j], count[j]});
        }
    } else {
        rc = _query(_text.data(), _off.data(), n, total.data(), missing.data());
        if (rc != HYPO_OK) return rc;
    }
    for (size_t i = 0; i < _who.size(); ++i) {
        Row& r = _rows[_who[i]];
        r.dt = total[2 * i]; r.dm = missing[2 * i]; r.pt = total[2 * i + 1]; r.pm = missing[2 * i + 1];
    }
    _text.clear(); _off.assign(1, 0); _who.clear();
    return HYPO_OK;
}

void QvReport::end() {
    if (_open) (void)_end();
    _open = false;
    std::string().swap(_text);
}

QvReport::Row QvReport::sums() const {
    Row s;
    for (const Row& r : _rows) { s.dm += r.dm; s.dt += r.dt; s.pm += r.pm; s.pt += r.pt; }
    return s;
}
std::string QvReport::draft_qv() const { const Row s = sums(); return qv_text(s.dm, s.dt, _k); }
std::string QvReport::polished_qv() const { const Row s = sums(); return qv_text(s.pm, s.pt, _k); }

void QvReport::write(std::ostream& os, const std::vector<std::string>& names) const {
    os << "#contig\tdraft_missing\tdraft_total\tdraft_qv\tpolished_missing\tpolished_total\tpolished_qv\n";
    auto row = [&](const std::string& name, const Row& r) {
        os << name << '\t' << r.dm << '\t' << r.dt << '\t' << qv_text(r.dm, r.dt, _k) << '\t' << r.pm << '\t' << r.pt << '\t' << qv_text(r.pm, r.pt, _k) << '\n';
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
