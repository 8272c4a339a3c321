// EditVcf.cpp — see EditVcf.hpp.
#include "EditVcf.hpp"
#include <dlfcn.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace hypo {

EditScriptsFn bind_edit_scripts() { return (EditScriptsFn)dlsym(RTLD_DEFAULT, "hypo_gpu_edit_scripts"); }

int edit_scripts_for(EditScriptsFn fn, const std::vector<std::unique_ptr<Contig>>& contigs, uint32_t c0, uint32_t c1, EditBatchResult& out) {
    const size_t nc = c1 - c0;
    out.units.assign(nc, {});
    out.first.assign(nc + 1, 0);
#pragma omp parallel for schedule(dynamic, 1)
    for (int64_t i = 0; i < (int64_t)nc; ++i) contigs[c0 + (size_t)i]->collect_units(out.units[(size_t)i]);
    for (size_t i = 0; i < nc; ++i) out.first[i + 1] = out.first[i] + out.units[i].size();
    const uint64_t nu = out.first[nc];
    if (nu >= (1ull << 32)) { std::fprintf(stderr, "[Hypo::Hypo] Error: %llu replacement units in one contig batch: use a smaller -p\n", (unsigned long long)nu); std::exit(1); }
    std::vector<uint64_t> a_off(nu + 1, 0), b_off(nu + 1, 0);
    std::vector<const EditUnit*> flat(nu);
    for (size_t i = 0; i < nc; ++i)
        for (size_t u = 0; u < out.units[i].size(); ++u) flat[out.first[i] + u] = &out.units[i][u];
    for (uint64_t u = 0; u < nu; ++u) { a_off[u + 1] = a_off[u] + (flat[u]->end - flat[u]->beg); b_off[u + 1] = b_off[u] + flat[u]->text.size(); }
    std::string a(a_off[nu], 'N'), b(b_off[nu], 'N');
    std::vector<uint32_t> owner(nu);
    for (size_t i = 0; i < nc; ++i) for (uint64_t u = out.first[i]; u < out.first[i + 1]; ++u) owner[u] = (uint32_t)i;
#pragma omp parallel for schedule(dynamic, 256)
    for (int64_t uu = 0; uu < (int64_t)nu; ++uu) {
        const uint64_t u = (uint64_t)uu;
        const Contig& ctg = *contigs[c0 + owner[u]];
        char* dst = &a[a_off[u]];
        for (uint32_t p = flat[u]->beg; p < flat[u]->end; ++p) *dst++ = ctg.draft_base(p);
        std::memcpy(&b[b_off[u]], flat[u]->text.data(), flat[u]->text.size());
    }
    HypoEditBatch in{};
    in.n_pairs = (uint32_t)nu; in.a = a.data(); in.a_off = a_off.data(); in.b = b.data(); in.b_off = b_off.data();
    std::vector<uint32_t> dist(nu ? nu : 1);
    out.run_off.assign(nu + 1, 0);
    // first guess: 4 runs per unit (the polishing runs measured 2.2 - 2.6), or the previous batch's rate with a quarter to spare; a
    // guess that is too small is answered with the size, and the retry only copies out what the device computed
    static double runs_per_unit = 4.0;
    out.runs.resize((size_t)(runs_per_unit * (double)nu) + 16);
    int rc = fn(&in, dist.data(), out.run_off.data(), out.runs.data(), out.runs.size());
    if (rc == HYPO_E_WORKSPACE) {
        out.runs.resize(out.run_off[nu]);
        rc = fn(&in, dist.data(), out.run_off.data(), out.runs.data(), out.runs.size());
    }
    if (rc == HYPO_OK && nu) runs_per_unit = std::max(4.0, 1.25 * (double)out.run_off[nu] / (double)nu);
    return rc;
}

void vcf_header(std::ostream& os, const std::string& reference, const std::vector<std::unique_ptr<Contig>>& contigs, bool kmer_filter) {
    os << "##fileformat=VCFv4.2\n##source=hypo\n##reference=" << reference << "\n";
    for (const auto& c : contigs) os << "##contig=<ID=" << c->get_name() << ",length=" << c->get_len() << ">\n";
    os << "##ALT=<ID=DEL,Description=\"Deletion\">\n"
          "##INFO=<ID=SVTYPE,Number=1,Type=String,Description=\"Type of structural variant\">\n"
          "##INFO=<ID=END,Number=1,Type=Integer,Description=\"End position of the variant\">\n";
    if (kmer_filter) os << "##FILTER=<ID=kmer,Description=\"rejected: adds k-mers that no read contains\">\n";
    os << "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n";
}

// Column stream of the contig: draft text between units is '=' columns, each unit its script.  A record is a maximal run of
// non-'=' columns; an empty REF or ALT takes the draft base before the run (after it, at position 0) on both sides; a record at 0
// padded with the base after it and the next record padded with that same base become one record.
void vcf_make_records(const Contig& ctg, const EditBatchResult& eb, size_t ci, VcfStats& st, VcfContigRecords& out) {
    const std::vector<EditUnit>& units = eb.units[ci];
    const uint64_t len = ctg.get_len();
    using Rec = VcfRec;
    out.recs.clear(); out.whole_del = false;
    std::vector<Rec> raw;
    Rec cur; bool open = false;
    auto close = [&] { if (open) { raw.push_back(std::move(cur)); cur = Rec(); open = false; } };
    uint64_t dp = 0, out_len = len;
    for (size_t u = 0; u < units.size(); ++u) {
        const EditUnit& U = units[u];
        out_len = out_len - (U.end - U.beg) + U.text.size();
        if (U.beg > dp) close();
        dp = U.beg;
        size_t tp = 0;
        const uint64_t g = eb.first[ci] + u;
        for (uint64_t r = eb.run_off[g]; r < eb.run_off[g + 1]; ++r) {
            const uint32_t n = eb.runs[r] >> 2, op = eb.runs[r] & 3u;
            if (op == 0) { if (n) close(); dp += n; tp += n; continue; }
            if (!open) { open = true; cur.rb = cur.re = dp; }
            if (op == 1 || op == 3) { if (tp + n > U.text.size()) break; cur.alt.append(U.text, tp, n); tp += n; }
            if (op == 1 || op == 2) dp += n;
            cur.re = dp;
            (op == 1 ? st.sub : op == 2 ? st.del : st.ins) += n;
        }
        if (dp != U.end || tp != U.text.size()) {
            std::fprintf(stderr, "[Hypo::Hypo] Error: contig %s: the edit script of unit [%u, %u) does not span it\n", ctg.get_name().c_str(), U.beg, U.end);
            std::exit(1);
        }
    }
    close();
    if (len > 0 && out_len == 0) {
        out.whole_del = true;
        ++st.records;
        return;
    }
    std::vector<Rec>& recs = out.recs;
    for (Rec& r : raw) {
        if (r.rb == r.re || r.alt.empty()) {
            if (r.rb > 0) { --r.rb; r.alt.insert(r.alt.begin(), ctg.draft_base(r.rb)); }
            else { r.alt.push_back(ctg.draft_base(r.re)); ++r.re; }
        }
        if (!recs.empty() && recs.back().re > r.rb) {
            Rec& p = recs.back();
            p.alt.append(r.alt, (size_t)(p.re - r.rb), std::string::npos);
            p.re = r.re;
            continue;
        }
        recs.push_back(std::move(r));
    }
    st.records += recs.size();
}

void vcf_write_records(std::ostream& os, const Contig& ctg, const VcfContigRecords& rs, const std::vector<uint8_t>* rejected) {
    const std::string& name = ctg.get_name();
    if (rs.whole_del) {
        os << name << "\t1\t.\t" << ctg.draft_base(0) << "\t<DEL>\t.\tPASS\tSVTYPE=DEL;END=" << ctg.get_len() << "\n";
        return;
    }
    std::string line;
    for (size_t i = 0; i < rs.recs.size(); ++i) {
        const VcfRec& r = rs.recs[i];
        line.clear();
        line += name; line += '\t'; line += std::to_string(r.rb + 1); line += "\t.\t";
        line += ctg.draft_segment((uint32_t)r.rb, (uint32_t)r.re);
        line += '\t'; line += r.alt; line += rejected && (*rejected)[i] ? "\t.\tkmer\t.\n" : "\t.\tPASS\t.\n";
        os << line;
    }
}

void vcf_records(std::ostream& os, const Contig& ctg, const EditBatchResult& eb, size_t ci, VcfStats& st) {
    VcfContigRecords rs;
    vcf_make_records(ctg, eb, ci, st, rs);
    vcf_write_records(os, ctg, rs, nullptr);
}

}  // namespace hypo
