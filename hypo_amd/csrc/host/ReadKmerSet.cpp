// ReadKmerSet.cpp — see ReadKmerSet.hpp.
#include "ReadKmerSet.hpp"
#include <dlfcn.h>

namespace hypo {

bool ReadKmerSet::bind() {
    _begin = (decltype(_begin))dlsym(RTLD_DEFAULT, "hypo_gpu_kset_begin");
    _add = (decltype(_add))dlsym(RTLD_DEFAULT, "hypo_gpu_kset_add");
    _size = (decltype(_size))dlsym(RTLD_DEFAULT, "hypo_gpu_kset_size");
    _end = (decltype(_end))dlsym(RTLD_DEFAULT, "hypo_gpu_kset_end");
    return have_set();
}

bool ReadKmerSet::bind_counts() {
    _counts_enable = (decltype(_counts_enable))dlsym(RTLD_DEFAULT, "hypo_gpu_kset_counts_enable");
    _spectrum = (decltype(_spectrum))dlsym(RTLD_DEFAULT, "hypo_gpu_kset_spectrum");
    _set_min_count = (decltype(_set_min_count))dlsym(RTLD_DEFAULT, "hypo_gpu_kset_min_count");
    return have_counts() && have_min_count();
}

bool ReadKmerSet::bind_track() {
    _track = (decltype(_track))dlsym(RTLD_DEFAULT, "hypo_gpu_kset_query_track");
    return have_track();
}

bool ReadKmerSet::bind_export() {
    _export = (decltype(_export))dlsym(RTLD_DEFAULT, "hypo_gpu_kset_export");
    return _export != nullptr;
}

bool ReadKmerSet::bind_import() {
    _import = (decltype(_import))dlsym(RTLD_DEFAULT, "hypo_gpu_kset_import");
    return _import != nullptr;
}

int ReadKmerSet::begin(uint32_t k, uint64_t expected_distinct, uint64_t max_bytes) {
    const int rc = _begin(k, expected_distinct, max_bytes);
    if (rc != HYPO_OK) return rc;
    _open = true; _k = k;
    return HYPO_OK;
}

int ReadKmerSet::enable_counts(uint32_t n_texts) { return _counts_enable(n_texts); }

ReadSink ReadKmerSet::sink() {
    ReadSink s;
    s.k = _k;
    s.add = [this](const char* p, uint64_t n) { return _add(p, n); };
    return s;
}

int ReadKmerSet::reads_done() { return _size(&_n_distinct, nullptr); }

uint32_t ReadKmerSet::valley(const uint64_t* h) {
    for (uint32_t c = 2; c < kRows - 1; ++c) if (h[c] <= h[c + 1]) return c;
    return 2;
}

int ReadKmerSet::spectrum(uint32_t text, std::vector<uint64_t>& hist) const {
    hist.assign((size_t)kRows * kCols, 0);
    return _spectrum(text, hist.data());
}

int ReadKmerSet::set_min_count(uint32_t given) {
    // no text has been marked yet: every key of the set is in column 0 of its count's row
    std::vector<uint64_t> hist;
    int rc = spectrum(0, hist);
    if (rc != HYPO_OK) return rc;
    uint64_t h[kRows];
    for (uint32_t c = 0; c < kRows; ++c) { h[c] = 0; for (uint32_t j = 0; j < kCols; ++j) h[c] += hist[(size_t)c * kCols + j]; }
    const uint32_t t = given ? given : valley(h);
    if ((rc = _set_min_count(t)) != HYPO_OK) return rc;
    _min_count = t; _n_reliable = 0;
    for (uint32_t c = t; c < kRows; ++c) _n_reliable += h[c];
    return HYPO_OK;
}

void ReadKmerSet::end() {
    if (_open) (void)_end();
    _open = false;
}

int ReadKmerSet::query_track(const std::string& text, const std::vector<uint64_t>& off, const uint8_t* want, Track& out) const {
    const uint32_t n = (uint32_t)(off.size() - 1);
    const size_t room = 1024 + text.size() / 1024;
    out.total.assign(n, 0); out.missing.assign(n, 0); out.iv_off.assign((size_t)n + 1, 0);
    out.start.assign(room, 0); out.end.assign(room, 0); out.count.assign(room, 0);
    auto call = [&] {
        return _track(text.data(), off.data(), n, want, out.total.data(), out.missing.data(), out.iv_off.data(), out.start.data(), out.end.data(), out.count.data(), out.start.size());
    };
    int rc = call();
    if (rc == HYPO_E_WORKSPACE) {
        out.start.resize(out.iv_off[n]); out.end.resize(out.iv_off[n]); out.count.resize(out.iv_off[n]);
        rc = call();
    }
    return rc;
}

}  // namespace hypo
