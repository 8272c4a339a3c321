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

bool ReadKmerSet::bind_depth() {
    _depth = (decltype(_depth))dlsym(RTLD_DEFAULT, "hypo_gpu_kset_query_depth");
    return have_depth();
}

uint32_t ReadKmerSet::peak(const uint64_t* h) {
    uint32_t best = 0;
    for (uint32_t c = valley(h); c < kRows - 1; ++c) if (h[c] > (best ? h[best] : 0)) best = c;
    return best;
}

int ReadKmerSet::query_depth(const std::string& text, const std::vector<uint64_t>& off, uint32_t bin, uint32_t plane, uint32_t unit, Depth& out,
                             size_t per_call) const {
    const size_t n = off.size() - 1;
    auto bins_of = [&](uint64_t len) { return (len + bin - 1) / bin; };
    out = Depth();
    Depth got;
    // one call over the sequences `o`; the first `keep` of its bins are the answer's next ones
    auto call = [&](const uint64_t* o, uint32_t n_seqs, uint64_t keep) {
        uint64_t n_bins = 0;
        for (uint32_t s = 0; s < n_seqs; ++s) n_bins += bins_of(o[s + 1] - o[s]);
        got.windows.assign(n_bins, 0); got.missing.assign(n_bins, 0); got.rated.assign(n_bins, 0); got.over.assign(n_bins, 0); got.under.assign(n_bins, 0);
        got.median.assign(n_bins, 0);
        const int rc = _depth(text.data(), o, n_seqs, bin, plane, unit, n_bins, got.windows.data(), got.missing.data(), got.rated.data(), got.over.data(),
                              got.under.data(), got.median.data());
        if (rc != HYPO_OK) return rc;
        if (keep > n_bins) keep = n_bins;
        out.windows.insert(out.windows.end(), got.windows.begin(), got.windows.begin() + keep);
        out.missing.insert(out.missing.end(), got.missing.begin(), got.missing.begin() + keep);
        out.rated.insert(out.rated.end(), got.rated.begin(), got.rated.begin() + keep);
        out.over.insert(out.over.end(), got.over.begin(), got.over.begin() + keep);
        out.under.insert(out.under.end(), got.under.begin(), got.under.begin() + keep);
        out.median.insert(out.median.end(), got.median.begin(), got.median.begin() + keep);
        return (int)HYPO_OK;
    };
    for (size_t s = 0; s < n;) {
        const uint64_t len = off[s + 1] - off[s];
        if (len > per_call) {                                    // one long sequence, in pieces of whole bins
            const uint64_t n_bins = bins_of(len);
            const uint64_t step = per_call > (uint64_t)bin + _k ? (per_call - (_k - 1)) / bin : 1;
            for (uint64_t j = 0; j < n_bins; j += step) {
                const uint64_t j1 = j + step < n_bins ? j + step : n_bins;
                const uint64_t lo = j * bin, hi = j1 == n_bins ? len : j1 * bin + (_k - 1) < len ? j1 * bin + (_k - 1) : len;
                const uint64_t o[2] = {off[s] + lo, off[s] + hi};
                if (const int rc = call(o, 1, j1 - j)) return rc;
            }
            ++s;
            continue;
        }
        size_t e = s + 1;                                        // whole sequences as far as they fit
        while (e < n && off[e + 1] - off[s] <= per_call) ++e;
        if (const int rc = call(off.data() + s, (uint32_t)(e - s), ~0ull)) return rc;
        s = e;
    }
    return HYPO_OK;
}

}  // namespace hypo
