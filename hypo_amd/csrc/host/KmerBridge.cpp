// KmerBridge.cpp — see KmerBridge.hpp.
#include "KmerBridge.hpp"
#include <dlfcn.h>
#include <algorithm>
#include <cctype>
#include <cstdio>

namespace hypo {

namespace {
bool is_base(char c) {
    switch (c) { case 'A': case 'C': case 'G': case 'T': case 'a': case 'c': case 'g': case 't': return true; default: return false; }
}
bool same_base(char a, char b) { return std::toupper((unsigned char)a) == std::toupper((unsigned char)b); }
struct Site { size_t contig; uint64_t n, a, b; uint32_t d0; };          // a, b: the anchors' positions in the call's text
}

static_assert(KmerBridge::kMaxHi + KmerBridge::kSlackHi <= HYPO_KSET_MAX_WALK && KmerBridge::kBudget <= HYPO_KSET_MAX_WALK_BUDGET, "the entry point's limits");

bool KmerBridge::bind() {
    _walks = (decltype(_walks))dlsym(RTLD_DEFAULT, "hypo_gpu_kset_query_walks");
    return _walks != nullptr;
}

bool KmerBridge::bind_vote() {
    _walk_sets = (decltype(_walk_sets))dlsym(RTLD_DEFAULT, "hypo_gpu_kset_query_walk_sets");
    return _walk_sets != nullptr;
}

int KmerBridge::push(uint32_t contig, const std::string& name, std::string draft, std::string text, const Emit& emit) {
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

int KmerBridge::flush(const Emit& emit) {
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
    // the sites (DESIGN.md "k-mer bridge"): the anchors lie inside the contig, at most _max apart, hold bases only, and the
    // neighbouring intervals are at least 2 bases away
    std::vector<Site> sites;
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t base = _pending[i].off, len = _pending[i].len;
        _stats.intervals += iv_off[i + 1] - iv_off[i];
        for (uint64_t j = iv_off[i]; j < iv_off[i + 1]; ++j) {
            const uint64_t s = start[j], e = end[j];
            if (s < 1 || e + 1 > len) continue;
            const uint64_t a = s - 1, b = e - k + 1, d0 = b - a;
            if (d0 < 2 || d0 > _max) continue;
            if (j > iv_off[i] && s - end[j - 1] < 2) continue;
            if (j + 1 < iv_off[i + 1] && start[j + 1] - e < 2) continue;
            const auto at = [&](uint64_t p) { return _text.begin() + (ptrdiff_t)(base + p); };
            if (!std::all_of(at(a), at(a + k), is_base) || !std::all_of(at(b), at(b + k), is_base)) continue;
            sites.push_back(Site{i, count[j], base + a, base + b, (uint32_t)d0});
        }
    }
    _stats.sites += sites.size();
    // the walks: one call (a site's walk takes HYPO_KSET_MAX_WALK bytes of the answer)
    const size_t ns = sites.size();
    std::vector<uint32_t> status(ns), steps(ns), wlen(ns);
    std::vector<uint8_t> walk(ns * HYPO_KSET_MAX_WALK);
    constexpr size_t kSitesPerCall = (size_t)1 << 18;
    for (size_t at = 0; at < ns; at += kSitesPerCall) {
        const size_t m = std::min(kSitesPerCall, ns - at);
        std::vector<uint64_t> from(m), to(m);
        std::vector<uint32_t> dlo(m), dhi(m);
        for (size_t s = 0; s < m; ++s) {
            const Site& st = sites[at + s];
            from[s] = st.a; to[s] = st.b;
            dlo[s] = st.d0 > _slack + 1 ? st.d0 - _slack : 1; dhi[s] = st.d0 + _slack;
        }
        rc = _walks(_text.data(), _text.size(), from.data(), to.data(), dlo.data(), dhi.data(), (uint32_t)m, kBudget, status.data() + at, steps.data() + at,
                    wlen.data() + at, walk.data() + at * HYPO_KSET_MAX_WALK);
        if (rc != HYPO_OK) return rc;
    }
    // --kmer-bridge-vote: the ambiguous sites once more, for up to 4 walks with their supports; a chosen site takes its place among
    // the unique ones, with the second search's steps and the chosen walk's bases
    std::vector<uint32_t> n_found, c_best, c_next;             // per site, under the vote: the walks found (1: unique), the two supports
    if (_ratio) {
        n_found.assign(ns, 1); c_best.assign(ns, 0); c_next.assign(ns, 0);
        std::vector<size_t> asked;
        for (size_t i = 0; i < ns; ++i) if (status[i] == HYPO_WALK_AMBIGUOUS) asked.push_back(i);
        _vstats.asked += asked.size();
        constexpr size_t W = HYPO_KSET_MAX_WALKS, kVotesPerCall = (size_t)1 << 16;
        std::vector<uint32_t> vst, vsteps, vn, vlen, vlow;
        std::vector<uint8_t> vwalk;
        for (size_t at = 0; at < asked.size(); at += kVotesPerCall) {
            const size_t m = std::min(kVotesPerCall, asked.size() - at);
            std::vector<uint64_t> from(m), to(m);
            std::vector<uint32_t> dlo(m), dhi(m);
            for (size_t j = 0; j < m; ++j) {
                const Site& st = sites[asked[at + j]];
                from[j] = st.a; to[j] = st.b;
                dlo[j] = st.d0 > _slack + 1 ? st.d0 - _slack : 1; dhi[j] = st.d0 + _slack;
            }
            vst.assign(m, 0); vsteps.assign(m, 0); vn.assign(m, 0); vlen.assign(m * W, 0); vlow.assign(m * W, 0); vwalk.assign(m * W * HYPO_KSET_MAX_WALK, 0);
            rc = _walk_sets(_text.data(), _text.size(), from.data(), to.data(), dlo.data(), dhi.data(), (uint32_t)m, kBudget, vst.data(), vsteps.data(), vn.data(),
                            vlen.data(), vlow.data(), vwalk.data());
            if (rc != HYPO_OK) return rc;
            for (size_t j = 0; j < m; ++j) {
                if (vst[j] == HYPO_WALK_MANY) { ++_vstats.many; continue; }
                if (vst[j] == HYPO_WALK_BUDGET) { ++_vstats.over_budget; continue; }
                // the best and the second best support (the first among equals: two equal supports are never far enough apart)
                size_t best = 0, next = W;
                const uint32_t nw = std::min<uint32_t>(vn[j], (uint32_t)W);
                for (size_t w = 1; w < nw; ++w) if (vlow[j * W + w] > vlow[j * W + best]) best = w;
                for (size_t w = 0; w < nw; ++w) if (w != best && (next == W || vlow[j * W + w] > vlow[j * W + next])) next = w;
                // the first search saw two walks arrive: a second one that sees fewer disagrees with it, and nothing it says is used
                if (vst[j] != HYPO_WALK_AMBIGUOUS || next == W) {
                    std::fprintf(stderr, "[Hypo::Hypo] Error: k-mer bridge vote: hypo_gpu_kset_query_walk_sets answers status %u with %u walks for a site that hypo_gpu_kset_query_walks "
                                         "found ambiguous (anchors at %llu and %llu)\n", vst[j], vn[j], (unsigned long long)from[j], (unsigned long long)to[j]);
                    return HYPO_E_INVALID;
                }
                if ((uint64_t)vlow[j * W + best] < (uint64_t)_ratio * vlow[j * W + next]) { ++_vstats.close; continue; }
                const size_t i = asked[at + j];
                ++_vstats.chosen;
                status[i] = HYPO_WALK_UNIQUE; steps[i] = vsteps[j]; wlen[i] = vlen[j * W + best];
                std::copy_n(vwalk.begin() + (ptrdiff_t)((j * W + best) * HYPO_KSET_MAX_WALK), wlen[i], walk.begin() + (ptrdiff_t)(i * HYPO_KSET_MAX_WALK));
                n_found[i] = nw; c_best[i] = vlow[j * W + best]; c_next[i] = vlow[j * W + next];
            }
        }
    }
    // the bridges go in contig by contig, in ascending order
    size_t s = 0;
    std::string out, fresh;
    for (uint32_t i = 0; i < n; ++i) {
        const Pending& p = _pending[i];
        out.clear();
        out.reserve(p.len + 64);
        uint64_t from = p.off;                                  // what lies before it is in `out`
        for (; s < ns && sites[s].contig == i; ++s) {
            if (status[s] == HYPO_WALK_AMBIGUOUS) ++_stats.ambiguous;
            if (status[s] == HYPO_WALK_BUDGET) ++_stats.over_budget;
            if (status[s] != HYPO_WALK_UNIQUE) continue;
            const Site& st = sites[s];
            // old = text[a, b + k), new = the left anchor and the walk: the common prefix goes, then the common suffix of the rest
            const uint64_t old_len = st.d0 + k, new_len = k + wlen[s];
            fresh.assign(_text, st.a, k);
            fresh.append((const char*)walk.data() + s * HYPO_KSET_MAX_WALK, wlen[s]);
            const char* old = _text.data() + st.a;
            uint64_t pre = 0, suf = 0;
            while (pre < old_len && pre < new_len && same_base(old[pre], fresh[pre])) ++pre;
            while (suf < old_len - pre && suf < new_len - pre && same_base(old[old_len - 1 - suf], fresh[new_len - 1 - suf])) ++suf;
            const uint64_t pos = st.a + pre, ref_len = old_len - pre - suf, alt_len = new_len - pre - suf;
            out.append(_text, from, pos - from);
            out.append(fresh, pre, alt_len);
            from = pos + ref_len;
            ++_stats.bridged; _stats.bases_out += ref_len; _stats.bases_in += alt_len; _stats.removed += st.n;
            _lines += p.name; _lines += '\t'; _lines += std::to_string(pos - p.off); _lines += '\t';
            if (ref_len) _lines.append(_text, pos, ref_len); else _lines += '.';
            _lines += '\t';
            if (alt_len) _lines.append(fresh, pre, alt_len); else _lines += '.';
            _lines += '\t'; _lines += std::to_string(st.n); _lines += '\t'; _lines += std::to_string(steps[s]);
            if (_ratio) {
                _lines += '\t'; _lines += std::to_string(n_found[s]); _lines += '\t';
                if (n_found[s] > 1) { _lines += std::to_string(c_best[s]); _lines += '/'; _lines += std::to_string(c_next[s]); } else _lines += '.';
            }
            _lines += '\n';
        }
        out.append(_text, from, p.off + p.len - from);
        rc = emit(p.contig, p.draft, out);
        if (rc != HYPO_OK) return rc;
    }
    _pending.clear(); _text.clear();
    return HYPO_OK;
}

void KmerBridge::write(std::ostream& os) const {
    os << "#contig\tpos\tref\talt\tmissing_kmers\tsteps" << (_ratio ? "\twalks\tsupport\n" : "\n") << _lines;
}

}  // namespace hypo
