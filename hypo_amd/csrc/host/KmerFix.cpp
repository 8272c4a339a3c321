// KmerFix.cpp — see KmerFix.hpp.
#include "KmerFix.hpp"
#include <dlfcn.h>
#include <algorithm>

namespace hypo {

namespace {
bool is_base(char c) {
    switch (c) { case 'A': case 'C': case 'G': case 'T': case 'a': case 'c': case 'g': case 't': return true; default: return false; }
}
struct Site { size_t contig; uint64_t start, n, lo, hi, c0, c1; };     // positions in the call's text; start: where the interval begins
}

bool KmerFix::bind() {
    _fixes = (decltype(_fixes))dlsym(RTLD_DEFAULT, "hypo_gpu_kset_query_fixes");
    return _fixes != nullptr;
}

int KmerFix::push(uint32_t contig, const std::string& name, std::string draft, std::string text, const Emit& emit) {
    if (!_pending.empty() && _text.size() + text.size() > ReadKmerSet::kTextPerCall) {
        const int rc = flush(emit);
        if (rc != HYPO_OK) return rc;
    }
    Pending p;
    p.contig = contig; p.name = name; p.draft = std::move(draft); p.off = _text.size(); p.len = text.size();
    if (_pending.empty()) _text = std::move(text); else _text += text;
    _pending.push_back(std::move(p));
    return HYPO_OK;
}

int KmerFix::flush(const Emit& emit) {
    if (_pending.empty()) return HYPO_OK;
    const uint32_t n = (uint32_t)_pending.size();
    const uint64_t k = _set.k();
    // the intervals of every text: one track query
    std::vector<uint64_t> off(n + 1);
    for (uint32_t i = 0; i < n; ++i) off[i] = _pending[i].off;
    off[n] = _text.size();
    ReadKmerSet::Track t;
    int rc = _set.query_track(_text, off, nullptr, t);
    if (rc != HYPO_OK) return rc;
    const std::vector<uint64_t> &iv_off = t.iv_off, &start = t.start, &end = t.end, &count = t.count;
    // the sites: rules (a) to (e) of DESIGN.md "k-mer fix"
    std::vector<Site> sites;
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t base = _pending[i].off, len = _pending[i].len;
        _stats.intervals += iv_off[i + 1] - iv_off[i];
        for (uint64_t j = iv_off[i]; j < iv_off[i + 1]; ++j) {
            const uint64_t s = start[j], e = end[j], width = e - s;
            if (width < k || width > 2 * k - 1 || count[j] != width - k + 1) continue;                          // (a)
            if (j > iv_off[i] && s - end[j - 1] < k - 1) continue;                                              // (b)
            if (j + 1 < iv_off[i + 1] && start[j + 1] - e < k - 1) continue;
            if (s + 1 < k || e + k - 1 > len) continue;                                                         // (c)
            const uint64_t lo = s + 1 - k, hi = e + k - 1, c0 = e - k, c1 = s + k;
            if (!std::all_of(_text.begin() + (ptrdiff_t)(base + lo), _text.begin() + (ptrdiff_t)(base + hi), is_base)) continue;   // (d)
            if (c1 - c0 > HYPO_KSET_MAX_FIX_REGION) continue;                                                   // (e)
            sites.push_back(Site{i, base + s, count[j], base + lo, base + hi, base + c0, base + c1});
        }
    }
    _stats.sites += sites.size();
    // every one-base edit of every region: one fixes call (at most 2^31 candidates a call, 276 a site)
    const size_t ns = sites.size();
    std::vector<uint32_t> best_cand(ns), zeros(ns);
    std::vector<uint64_t> best_missing(ns);
    constexpr size_t kSitesPerCall = (size_t)1 << 22;
    for (size_t at = 0; at < ns; at += kSitesPerCall) {
        const size_t m = std::min(kSitesPerCall, ns - at);
        std::vector<uint64_t> lo(m), hi(m), c0(m), c1(m), none_total(m), none_missing(m), best_total(m);
        for (size_t s = 0; s < m; ++s) { lo[s] = sites[at + s].lo; hi[s] = sites[at + s].hi; c0[s] = sites[at + s].c0; c1[s] = sites[at + s].c1; }
        rc = _fixes(_text.data(), _text.size(), lo.data(), hi.data(), c0.data(), c1.data(), (uint32_t)m, none_total.data(), none_missing.data(), best_cand.data() + at,
                    best_total.data(), best_missing.data() + at, zeros.data() + at, nullptr, nullptr);
        if (rc != HYPO_OK) return rc;
    }
    // the fixes go in contig by contig, in ascending order
    size_t s = 0;
    std::string fixed;
    for (uint32_t i = 0; i < n; ++i) {
        const Pending& p = _pending[i];
        fixed.clear();
        fixed.reserve(p.len + 64);
        uint64_t from = p.off;                                  // what lies before it is in `fixed`
        for (; s < ns && sites[s].contig == i; ++s) {
            if (zeros[s] >= 2) ++_stats.ambiguous;
            if (best_missing[s] != 0 || zeros[s] != 1) continue;
            const Site& st = sites[s];
            const uint32_t w = (uint32_t)(st.c1 - st.c0);
            uint32_t j = best_cand[s] - 1;                       // (the unedited span is never the best: it is not canonical)
            uint64_t pos;
            const char* kind;
            char ref = '.', alt = '.';
            if (j < 4 * w) { pos = st.c0 + j / 4; kind = "sub"; ref = _text[pos]; alt = "ACGT"[j % 4]; ++_stats.sub; }
            else if ((j -= 4 * w) < w) { pos = st.c0 + j; kind = "del"; ref = _text[pos]; ++_stats.del; }
            else { j -= w; pos = st.c0 + 1 + j / 4; kind = "ins"; alt = "ACGT"[j % 4]; ++_stats.ins; }
            fixed.append(_text, from, pos - from);
            if (alt != '.') fixed += alt;
            from = ref != '.' ? pos + 1 : pos;
            ++_stats.fixed; _stats.removed += st.n;
            _lines += p.name; _lines += '\t'; _lines += std::to_string(pos - p.off); _lines += '\t'; _lines += kind; _lines += '\t'; _lines += ref; _lines += '\t';
            _lines += alt; _lines += '\t'; _lines += std::to_string(st.n); _lines += '\n';
        }
        fixed.append(_text, from, p.off + p.len - from);
        rc = emit(p.contig, p.draft, fixed);
        if (rc != HYPO_OK) return rc;
    }
    _pending.clear(); _text.clear();
    return HYPO_OK;
}

void KmerFix::write(std::ostream& os) const {
    os << "#contig\tpos\tkind\tref\talt\tmissing_kmers\n" << _lines;
}

}  // namespace hypo
