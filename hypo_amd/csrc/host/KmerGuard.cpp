// KmerGuard.cpp — see KmerGuard.hpp.
#include "KmerGuard.hpp"
#include <dlfcn.h>
#include <algorithm>

namespace hypo {

bool KmerGuard::bind() {
    _spans = (decltype(_spans))dlsym(RTLD_DEFAULT, "hypo_gpu_kset_query_spans");
    return _spans != nullptr;
}

bool KmerGuard::bind_variants(uint32_t max_records) {
    _variants = (decltype(_variants))dlsym(RTLD_DEFAULT, "hypo_gpu_kset_query_variants");
    _max_records = max_records;
    return _variants != nullptr;
}

void KmerGuard::clusters_of(const std::vector<VcfRec>& recs, uint32_t k, std::vector<Cluster>& out) {
    out.clear();
    int64_t shift = 0;                                       // polished position - draft position before the record in hand
    for (size_t i = 0; i < recs.size(); ++i) {
        const VcfRec& r = recs[i];
        const int64_t delta = (int64_t)r.alt.size() - (int64_t)(r.re - r.rb);
        if (out.empty() || r.rb - out.back().e >= (uint64_t)(k - 1)) {
            Cluster c;
            c.r0 = i; c.b = r.rb; c.qb = (uint64_t)((int64_t)r.rb + shift);
            out.push_back(c);
        }
        shift += delta;
        Cluster& c = out.back();
        c.r1 = i + 1; c.e = r.re; c.qe = (uint64_t)((int64_t)r.re + shift);
    }
}

std::string KmerGuard::apply(const std::string& draft, const std::vector<VcfRec>& recs, const std::vector<uint8_t>& rejected) {
    std::string out;
    out.reserve(draft.size() + draft.size() / 64);
    uint64_t at = 0;
    for (size_t i = 0; i < recs.size(); ++i) {
        if (rejected[i]) continue;
        out.append(draft, at, recs[i].rb - at);
        out += recs[i].alt;
        at = recs[i].re;
    }
    out.append(draft, at, std::string::npos);
    return out;
}

int KmerGuard::run_batch(const std::vector<std::unique_ptr<Contig>>& contigs, uint32_t c0, uint32_t c1, const EditBatchResult& eb, VcfStats& vst, const Emit& emit) {
    const uint32_t k = _set.k();
    for (uint32_t c = c0; c < c1; ++c) {
        const Contig& ctg = *contigs[c];
        Pending p;
        p.contig = c;
        vcf_make_records(ctg, eb, c - c0, vst, p.recs);
        clusters_of(p.recs.recs, k, p.clusters);              // (none for a contig written as nothing: its <DEL> record is not guarded)
        std::string d = ctg.draft_segment(0, (uint32_t)ctg.get_len()), q = ctg.polished_text();
        uint64_t variants = 0;                                   // by record: what the contig adds to the call's sum of 2^n
        if (by_record()) for (const Cluster& cl : p.clusters) variants += cl.r1 - cl.r0 <= _max_records ? 1ull << (cl.r1 - cl.r0) : 2;
        if (!_pending.empty() && (_text.size() + d.size() + q.size() > ReadKmerSet::kTextPerCall || _lo.size() + 2 * p.clusters.size() >= (1ull << 32) ||
                                  _eb.size() + p.recs.recs.size() >= (1ull << 32) || _n_variants + variants >= (1ull << 31))) {
            const int rc = flush(emit);
            if (rc != HYPO_OK) return rc;
        }
        p.d_off = _text.size(); p.d_len = d.size(); _text += d;
        if (by_record()) {
            _n_variants += variants;
            // one site per cluster: its records are the edits, or (more than N records) one edit that is its whole polished span
            p.span0 = _lo.size();
            const uint64_t flank = k - 1;
            for (const Cluster& cl : p.clusters) {
                _lo.push_back(p.d_off + (cl.b > flank ? cl.b - flank : 0)); _hi.push_back(p.d_off + std::min<uint64_t>(p.d_len, cl.e + flank));
                if (_edit_off.empty()) _edit_off.push_back(0);
                auto edit = [&](uint64_t b, uint64_t e, const char* alt, size_t n) {
                    _eb.push_back(p.d_off + b); _ee.push_back(p.d_off + e); _ao.push_back(_alts.size()); _al.push_back((uint32_t)n);
                    _alts.append(alt, n);
                };
                if (cl.r1 - cl.r0 <= _max_records)
                    for (size_t i = cl.r0; i < cl.r1; ++i) edit(p.recs.recs[i].rb, p.recs.recs[i].re, p.recs.recs[i].alt.data(), p.recs.recs[i].alt.size());
                else
                    edit(cl.b, cl.e, q.data() + cl.qb, (size_t)(cl.qe - cl.qb));
                _edit_off.push_back((uint32_t)_eb.size());
            }
            p.p_len = q.size();
            _polished.push_back(std::move(q));
            _pending.push_back(std::move(p));
            continue;
        }
        p.p_off = _text.size(); p.p_len = q.size(); _text += q;
        p.span0 = _lo.size();
        const uint64_t flank = k - 1;
        for (const Cluster& cl : p.clusters) {
            _lo.push_back(p.d_off + (cl.b > flank ? cl.b - flank : 0)); _hi.push_back(p.d_off + std::min<uint64_t>(p.d_len, cl.e + flank));
            _lo.push_back(p.p_off + (cl.qb > flank ? cl.qb - flank : 0)); _hi.push_back(p.p_off + std::min<uint64_t>(p.p_len, cl.qe + flank));
        }
        _pending.push_back(std::move(p));
    }
    return flush(emit);
}

int KmerGuard::flush_by_record(const Emit& emit) {
    const size_t n_sites = _lo.size();
    std::vector<uint32_t> best_mask(n_sites ? n_sites : 1);
    std::vector<uint64_t> best_total(best_mask.size()), best_missing(best_mask.size());
    if (n_sites) {
        const int rc = _variants(_text.data(), _text.size(), _alts.data(), _alts.size(), _lo.data(), _hi.data(), _edit_off.data(), (uint32_t)n_sites, _eb.data(), _ee.data(),
                                 _ao.data(), _al.data(), best_mask.data(), best_total.data(), best_missing.data(), nullptr, nullptr);
        if (rc != HYPO_OK) return rc;
    }
    std::vector<uint8_t> rejected;
    for (size_t pi = 0; pi < _pending.size(); ++pi) {
        const Pending& p = _pending[pi];
        rejected.assign(p.recs.recs.size(), 0);
        bool any = false;
        for (size_t i = 0; i < p.clusters.size(); ++i) {
            const Cluster& cl = p.clusters[i];
            const size_t n = cl.r1 - cl.r0;
            const uint32_t mask = best_mask[p.span0 + i];
            ++_stats.clusters; _stats.records += n; ++_stats.by_size[n <= _max_records ? n : 0];
            size_t n_rej = 0;
            for (size_t j = 0; j < n; ++j) {
                const bool keep = n <= _max_records ? (mask >> j) & 1u : mask != 0;     // (decided whole: the site's only edit)
                if (!keep) { rejected[cl.r0 + j] = 1; ++n_rej; }
            }
            if (!n_rej) continue;
            any = true;
            _stats.rejected_records += n_rej;
            ++(n_rej == n ? _stats.rejected_clusters : _stats.partial_clusters);
        }
        const std::string draft = _text.substr(p.d_off, p.d_len);
        const int rc = emit(p.contig, draft, any ? apply(draft, p.recs.recs, rejected) : _polished[pi], p.recs, rejected);
        if (rc != HYPO_OK) return rc;
    }
    _pending.clear(); _lo.clear(); _hi.clear(); _text.clear();
    _alts.clear(); _edit_off.clear(); _al.clear(); _eb.clear(); _ee.clear(); _ao.clear(); _polished.clear(); _n_variants = 0;
    return HYPO_OK;
}

int KmerGuard::flush(const Emit& emit) {
    if (_pending.empty()) return HYPO_OK;
    if (by_record()) return flush_by_record(emit);
    std::vector<uint64_t> total(_lo.size() ? _lo.size() : 1), missing(total.size());
    if (!_lo.empty()) {
        const int rc = _spans(_text.data(), _text.size(), _lo.data(), _hi.data(), (uint32_t)_lo.size(), total.data(), missing.data());
        if (rc != HYPO_OK) return rc;
    }
    std::vector<uint8_t> rejected;
    for (const Pending& p : _pending) {
        rejected.assign(p.recs.recs.size(), 0);
        bool any = false;
        for (size_t i = 0; i < p.clusters.size(); ++i) {
            const Cluster& cl = p.clusters[i];
            const uint64_t r_c = missing[p.span0 + 2 * i], a_c = missing[p.span0 + 2 * i + 1];
            ++_stats.clusters; _stats.records += cl.r1 - cl.r0;
            if (a_c <= r_c) continue;                            // (a tie: the polish is trusted)
            ++_stats.rejected_clusters; _stats.rejected_records += cl.r1 - cl.r0;
            std::fill(rejected.begin() + (ptrdiff_t)cl.r0, rejected.begin() + (ptrdiff_t)cl.r1, (uint8_t)1);
            any = true;
        }
        const std::string draft = _text.substr(p.d_off, p.d_len);
        const int rc = emit(p.contig, draft, any ? apply(draft, p.recs.recs, rejected) : _text.substr(p.p_off, p.p_len), p.recs, rejected);
        if (rc != HYPO_OK) return rc;
    }
    _pending.clear(); _lo.clear(); _hi.clear(); _text.clear();
    return HYPO_OK;
}

}  // namespace hypo
