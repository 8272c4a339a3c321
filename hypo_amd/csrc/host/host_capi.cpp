// host_capi.cpp — C entry points over the C++ host mirror so that tests can drive it like the reference's
// own classes (same call sequence as oracle/ref_harness.cpp uses on the real reference).
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#include "SeqIO.hpp"
#include "Contig.hpp"
#include "Window.hpp"
#include "SolidBuild.hpp"
#include "CtxPlan.hpp"
#include "../edit_kernel.hpp"

using namespace hypo;

// What Alignment::update_solidkmers_support / update_minimisers_support read of a Contig, put there from the flat arrays the
// C-ABI of the device votes takes (include/hypo_gpu.h) instead of by a scan and prepare_for_division.
namespace hypo {
struct VoteTables {
    static void set_solid(Contig& c, uint64_t n_solid, const uint32_t* spos, const uint64_t* kids) {
        for (uint64_t i = 0; i < n_solid; ++i) c._solid_pos.set(spos[i]);
        c._solid_pos.init_support();
        c._kids.assign(kids, kids + n_solid);
        c._n_solid = n_solid;
        c._kcov.assign(n_solid, 0); c._ksup.assign(n_solid, 0);
    }
    static void get_solid(const Contig& c, uint32_t* cov, uint32_t* sup) {
        std::memcpy(cov, c._kcov.data(), c._kcov.size() * 4); std::memcpy(sup, c._ksup.data(), c._ksup.size() * 4);
    }
    // borders [n_borders]: the set bits of _reg_pos; entries of MWMinimiserInfo x of the contig: [off[x], off[x + 1]) of rel_pos / minimisers
    static void set_mega(Contig& c, const uint32_t* borders, uint32_t n_borders, bool even, uint32_t n_info, const uint32_t* off, const uint32_t* rel_pos, const uint32_t* minimisers) {
        for (uint32_t i = 0; i < n_borders; ++i) c._reg_pos.set(borders[i]);
        c._reg_pos.init_support();
        c._is_win_even = even;
        c._minimserinfo.assign(n_info, MWMinimiserInfo());
        for (uint32_t x = 0; x < n_info; ++x) {
            MWMinimiserInfo& mi = c._minimserinfo[x];
            mi.rel_pos.assign(rel_pos + off[x], rel_pos + off[x + 1]);
            mi.minimisers.assign(minimisers + off[x], minimisers + off[x + 1]);
            mi.coverage.assign(mi.rel_pos.size(), 0); mi.support.assign(mi.rel_pos.size(), 0);
        }
    }
    static void get_mega(const Contig& c, uint32_t n_info, const uint32_t* off, uint32_t* cov, uint32_t* sup) {
        for (uint32_t x = 0; x < n_info; ++x) {
            const MWMinimiserInfo& mi = c._minimserinfo[x];
            if (mi.coverage.empty()) continue;
            std::memcpy(cov + off[x], mi.coverage.data(), mi.coverage.size() * 4); std::memcpy(sup + off[x], mi.support.data(), mi.support.size() * 4);
        }
    }
};

// What Alignment::find_short_arms / find_long_arms and Contig::fill_short_windows / fill_long_windows read of a Contig, put there from
// the flat arrays of HypoArmsRegions (include/hypo_gpu.h) instead of by divide_into_regions / prepare_long_windows.
struct ArmTables {
    // SHORT: _reg_pos / _reg_type / _reg_info / _anchor_kmers and a SHORT Window per region that is neither SR nor MSR
    static void set_short(Contig& c, uint32_t nr, const uint32_t* start, const uint8_t* type, const uint32_t* info, uint64_t n_anchor, const uint64_t* anchors) {
        for (uint32_t i = 0; i <= nr; ++i) c._reg_pos.set(start[i]);
        c._reg_pos.init_support();
        c._reg_type.clear();
        for (uint32_t i = 0; i <= nr; ++i) c._reg_type.push_back((RegionType)type[i]);
        c._reg_info.assign(info, info + nr + 1);
        c._anchor_kmers.assign(anchors, anchors + n_anchor);
        c._pwindows.clear(); c._pwindows.resize((size_t)nr + 1);
        for (uint32_t i = 0; i < nr; ++i)
            if (c._reg_type[i] != RegionType::SR && c._reg_type[i] != RegionType::MSR) c._pwindows[i].reset(new Window(c._pseq, start[i], start[i + 1], WindowType::SHORT));
    }
    // LONG: the pseudo tables with the identity as _true_reg_id and a LONG Window per LONG region
    static void set_long(Contig& c, uint32_t nr, const uint32_t* start, const uint8_t* type) {
        c._pseudo_reg_pos = BitVec((uint64_t)c._len + 1);
        for (uint32_t i = 0; i <= nr; ++i) c._pseudo_reg_pos.set(start[i]);
        c._pseudo_reg_pos.init_support();
        c._pseudo_reg_type.clear(); c._true_reg_id.clear(); c._reg_type.clear();
        for (uint32_t i = 0; i <= nr; ++i) { c._pseudo_reg_type.push_back((RegionType)type[i]); c._reg_type.push_back((RegionType)type[i]); c._true_reg_id.push_back(i); }
        c._pwindows.clear(); c._pwindows.resize((size_t)nr + 1);
        for (uint32_t i = 0; i < nr; ++i)
            if (c._pseudo_reg_type[i] == RegionType::LONG) c._pwindows[i].reset(new Window(c._pseq, start[i], start[i + 1], WindowType::LONG));
    }
};
}  // namespace hypo

// the arms both exports return: per region whether a window remains, internal / prefix / suffix / empty, and Window::dump_text()
// ("draft|I:arm..|P:arm..|S:arm..") of the remaining windows, one per line in region order.  The number of bytes, -2: text too small
static long arms_report(const Contig& c, uint32_t nr, uint8_t* valid, uint32_t* counts, char* text, long cap) {
    long at = 0;
    for (uint32_t i = 0; i < nr; ++i) {
        valid[i] = c.is_valid_window(i) ? 1 : 0;
        counts[4 * i] = counts[4 * i + 1] = counts[4 * i + 2] = counts[4 * i + 3] = 0;
        if (!valid[i]) continue;
        const Window& w = *c.window(i);
        unsigned n[4] = {0, 0, 0, 0};
        std::sscanf(w.dump_counts().c_str(), "%u\t%u\t%u\t%u", &n[0], &n[1], &n[2], &n[3]);
        for (int j = 0; j < 4; ++j) counts[4 * i + j] = n[j];
        const std::string t = w.dump_text();
        if (at + (long)t.size() + 1 > cap) return -2;
        std::memcpy(text + at, t.data(), t.size()); at += (long)t.size(); text[at++] = '\n';
    }
    return at;
}
// an Alignment per record, in file order (file_rank NULL: the order given)
static bool arms_alignments(uint64_t total_len, uint32_t n, const uint32_t* rb, const uint32_t* re, const uint32_t* qae, const uint64_t* seq_off, const uint8_t* reads2,
                            const uint32_t* cigar_off, const uint32_t* cigar, const uint32_t* file_rank, std::vector<std::unique_ptr<Alignment>>& out) {
    out.clear(); out.resize(n);
    for (uint32_t a = 0; a < n; ++a) {
        const uint32_t at = file_rank ? file_rank[a] : a;
        if (re[a] <= rb[a] || re[a] > total_len || at >= n || out[at]) return false;
        out[at].reset(new Alignment(rb[a], re[a], qae[a], reads2 + seq_off[a], cigar + cigar_off[a], cigar_off[a + 1] - cigar_off[a]));
    }
    return true;
}
// the contig as text from its PackedSeq<4> bytes
static std::string arms_contig_text(const uint8_t* contig4, uint64_t total_len) {
    std::string s((size_t)total_len, 'N');
    for (uint64_t p = 0; p < total_len; ++p) { const unsigned c = (contig4[p >> 1] >> (4 - 4 * (p & 1))) & 15u; s[(size_t)p] = "ACGTN"[c < 4 ? c : 4]; }
    return s;
}

extern "C" {

// Alignment::find_short_arms of every record in file order, then Contig::fill_short_windows, over the flat tables hypo_gpu_arms_build
// takes (include/hypo_gpu.h; the tables must be consistent: tests/arms_cases.py check_tables).  OUT valid [n_regions], counts
// [4 * n_regions], text (see arms_report).  The number of text bytes; -1: a record does not fit; -2: text too small
long hypo_host_short_arms(uint32_t n_regions, const uint32_t* start, const uint8_t* type, const uint32_t* info, uint64_t n_anchor, const uint64_t* anchors, uint32_t k,
                          const uint8_t* contig4, uint32_t n_reads, const uint32_t* rb, const uint32_t* re, const uint32_t* qae, const uint64_t* seq_off, const uint8_t* reads2,
                          const uint32_t* cigar_off, const uint32_t* cigar, const uint32_t* file_rank, uint8_t* valid, uint32_t* counts, char* text, long cap) {
    const uint64_t total_len = start[n_regions];
    Contig c(0, "arms", arms_contig_text(contig4, total_len));
    ArmTables::set_short(c, n_regions, start, type, info, n_anchor, anchors);
    std::vector<std::unique_ptr<Alignment>> al;
    if (!arms_alignments(total_len, n_reads, rb, re, qae, seq_off, reads2, cigar_off, cigar, file_rank, al)) return -1;
    for (auto& a : al) a->find_short_arms(k, c);
    c.fill_short_windows(al);
    return arms_report(c, n_regions, valid, counts, text, cap);
}

// Alignment::find_long_arms of every record in file order, then Contig::fill_long_windows, over the pseudo regions hypo_gpu_arms_build_long takes
long hypo_host_long_arms(uint32_t n_regions, const uint32_t* start, const uint8_t* type, const uint8_t* contig4, uint32_t n_reads, const uint32_t* rb, const uint32_t* re,
                         const uint32_t* qae, const uint64_t* seq_off, const uint8_t* reads2, const uint32_t* cigar_off, const uint32_t* cigar, const uint32_t* file_rank,
                         uint8_t* valid, uint32_t* counts, char* text, long cap) {
    const uint64_t total_len = start[n_regions];
    Contig c(0, "arms", arms_contig_text(contig4, total_len));
    ArmTables::set_long(c, n_regions, start, type);
    std::vector<std::unique_ptr<Alignment>> al;
    if (!arms_alignments(total_len, n_reads, rb, re, qae, seq_off, reads2, cigar_off, cigar, file_rank, al)) return -1;
    for (auto& a : al) a->find_long_arms(c);
    c.fill_long_windows(al);
    return arms_report(c, n_regions, valid, counts, text, cap);
}

int hypo_host_set_scores(const int8_t sc[6]) {
    ScoreParams sp{sc[0], sc[1], sc[2], sc[3], sc[4], sc[5]};
    Window::prepare_for_poa(sp, 1);
    return 0;
}

// n windows given as flat string arrays; arms of window w are [arm_first[w], arm_first[w+1]) with counts per kind.
// out: consensus strings concatenated, lens per window; kept flags per arm (LONG windows filter arms).
int hypo_host_windows(int n, const int* is_long, const char* const* drafts, const int* ni, const int* np, const int* ns,
                      const int* n_empty, const char* const* arms, char* out, long out_cap, int* out_len,
                      unsigned char* kept, int batched) {
    std::vector<std::unique_ptr<Window>> ws;
    size_t a = 0;
    for (int w = 0; w < n; ++w) {
        std::string d(drafts[w]);
        PackedSeq<4> pd(d);
        ws.emplace_back(new Window(pd, 0, d.size(), is_long[w] ? WindowType::LONG : WindowType::SHORT));
        Window& W = *ws.back();
        for (int i = 0; i < ni[w]; ++i, ++a) { auto b = W.get_num_internal(); W.add_internal(PackedSeq<2>(std::string(arms[a]))); if (kept) kept[a] = W.get_num_internal() != b; }
        for (int i = 0; i < np[w]; ++i, ++a) { auto b = W.get_num_pre(); W.add_prefix(PackedSeq<2>(std::string(arms[a]))); if (kept) kept[a] = W.get_num_pre() != b; }
        for (int i = 0; i < ns[w]; ++i, ++a) { auto b = W.get_num_suf(); W.add_suffix(PackedSeq<2>(std::string(arms[a]))); if (kept) kept[a] = W.get_num_suf() != b; }
        for (int i = 0; i < n_empty[w]; ++i) W.add_empty();
    }
    if (batched) {
        std::vector<Window*> ptrs;
        for (auto& w : ws) ptrs.push_back(w.get());
        const int rc = Window::generate_consensus_batch(ptrs);
        if (rc != HYPO_OK) return rc;
    } else {
        for (auto& w : ws) w->generate_consensus(0);
    }
    long o = 0;
    for (int w = 0; w < n; ++w) {
        const std::string c = ws[w]->get_consensus();
        if (o + (long)c.size() > out_cap) return -100;
        std::memcpy(out + o, c.data(), c.size());
        out_len[w] = (int)c.size();
        o += (long)c.size();
    }
    return 0;
}

// Filter::initialise + is_good without a device (CPU test of the host logic)
int hypo_host_filter(const char* draft, int n_arms, const char* const* arms, unsigned char* good) {
    Filter f;
    f.initialise(std::string(draft));
    for (int i = 0; i < n_arms; ++i) good[i] = f.is_good(std::string(arms[i])) ? 1 : 0;
    return 0;
}

int hypo_host_pack_roundtrip(int nb, const char* text, char* out, int cap) {
    std::string u;
    if (nb == 2) u = PackedSeq<2>(std::string(text)).unpack(); else u = PackedSeq<4>(std::string(text)).unpack();
    if ((int)u.size() > cap) return -1;
    std::memcpy(out, u.data(), u.size());
    return (int)u.size();
}

// Contig::find_solid_pos + rank/select spot checks
int hypo_host_contig_scan(const char* seq, unsigned k, const uint64_t* words, uint64_t n_words,
                          uint64_t* n_solid, uint64_t* kids_out, uint64_t kids_cap,
                          const uint64_t* rank_q, uint64_t* rank_a, int n_rank,
                          const uint64_t* sel_q, uint64_t* sel_a, int n_sel) {
    SolidKmers sk; sk.k = k; sk.words.assign(words, words + n_words);
    Contig c(0, "ctg test", std::string(seq));
    const int rc = c.find_solid_pos(sk);
    if (rc != HYPO_OK) return rc;
    *n_solid = c.get_num_solid();
    for (uint64_t i = 0; i < c.get_num_solid() && i < kids_cap; ++i) kids_out[i] = c.kid_at(i);
    for (int i = 0; i < n_rank; ++i) rank_a[i] = c.rank(rank_q[i]);
    for (int i = 0; i < n_sel; ++i) sel_a[i] = c.select(sel_q[i]);
    return 0;
}

// read_fastx through the mapped reader (line_by_line = 0) or the line-by-line one: "name\tsequence\n" per record into out; the number of
// bytes, -1 when the file is not FASTA / FASTQ, -2 when out is too small
int hypo_host_read_fastx(const char* path, int line_by_line, char* out, int cap) {
    std::vector<hypo::FastaRecord> recs;
    if (!hypo::read_fastx(path, recs, line_by_line == 0)) return -1;
    size_t at = 0;
    for (const auto& r : recs) {
        const size_t need = r.name.size() + 1 + r.seq.size() + 1;
        if (at + need > (size_t)cap) return -2;
        std::memcpy(out + at, r.name.data(), r.name.size()); at += r.name.size(); out[at++] = '\t';
        std::memcpy(out + at, r.seq.data(), r.seq.size()); at += r.seq.size(); out[at++] = '\n';
    }
    return (int)at;
}

// find_cutoffs (SolidBuild.cpp) on hist[0 .. n_bins): out = {err, mean, lower, upper}; 0, or -1 when the reference's result is undefined
// (no maximum after the error threshold)
int hypo_host_solid_cutoffs(const uint64_t* hist, uint32_t n_bins, uint32_t* out) {
    std::vector<uint64_t> h(hist, hist + n_bins);
    hypo::CutOffs c;
    if (!hypo::find_cutoffs(h, c)) return -1;
    out[0] = c.err; out[1] = c.mean; out[2] = c.lower; out[3] = c.upper;
    return 0;
}

// the whole construction of a run without -i (build_solid_kmers: parser, device counting, cut-offs, set) over n read files on the
// calling thread's device context.  words: 4^k / 64 words; hist: 4c + 1 bins; cut: {err, mean, lower, upper}; counts: {set bits,
// canonical solid k-mers, sequence bytes sent to the device, bytes of the read files}; times: {parse, count, histogram, set, total}
// in seconds.  Returns SOLID_* (0 = ok, 2 = the cut-offs are undefined); the reason of a failure goes to err (err_cap bytes).
int hypo_host_solid_build(const char* const* paths, int n, uint32_t k, uint32_t coverage, uint64_t* words, uint64_t* hist,
                          uint32_t* cut, uint64_t* counts, double* times, char* err, int err_cap) {
    std::vector<std::string> files(paths, paths + n);
    hypo::SolidKmers sk;
    hypo::SolidBuildStats st;
    std::string e;
    const int rc = hypo::build_solid_kmers(files, k, coverage, 1, sk, st, e);
    if (err && err_cap > 0) { std::strncpy(err, e.c_str(), (size_t)err_cap - 1); err[err_cap - 1] = 0; }
    if (hist) for (size_t i = 0; i < st.hist.size(); ++i) hist[i] = st.hist[i];
    if (rc != hypo::SOLID_OK) return rc;
    if (words) std::memcpy(words, sk.words.data(), sk.words.size() * 8);
    cut[0] = st.cut.err; cut[1] = st.cut.mean; cut[2] = st.cut.lower; cut[3] = st.cut.upper;
    counts[0] = st.n_bits; counts[1] = st.n_canonical; counts[2] = st.seq_bytes; counts[3] = st.file_bytes;
    times[0] = st.parse_s; times[1] = st.count_s; times[2] = st.hist_s; times[3] = st.fill_s; times[4] = st.total_s;
    return rc;
}

// plan_contexts (CtxPlan.hpp): which context works on which contigs of the batch [initial_cid, final_cid); n_reads and contig_len per
// contig of the batch.  out: {c0, c1, piece, own0, own1} per context
int hypo_host_plan_contexts(uint32_t initial_cid, uint32_t final_cid, int n_ctx, const uint64_t* n_reads, const uint32_t* contig_len,
                            int split_batch, int allow_pieces, uint32_t* out) {
    const std::vector<hypo::CtxWork> work = hypo::plan_contexts(initial_cid, final_cid, n_ctx, n_reads, contig_len, split_batch != 0, allow_pieces != 0);
    for (const hypo::CtxWork& w : work) { *out++ = w.c0; *out++ = w.c1; *out++ = w.piece ? 1 : 0; *out++ = w.own0; *out++ = w.own1; }
    return 0;
}

// Alignment::update_solidkmers_support of every read over one coordinate space of total_len bases whose solid k-mers are given
// as hypo_gpu_support_kmers takes them (spos ascending, kids); the reads as hypo_gpu_reads_upload takes them.  OUT coverage /
// support [n_solid].  -1: a table or a read does not fit the coordinate space.
int hypo_host_kmer_votes(uint32_t k, uint64_t total_len, uint64_t n_solid, const uint32_t* spos, const uint64_t* kids, uint32_t n_reads, const uint32_t* rb,
                         const uint32_t* re, const uint32_t* qae, const uint64_t* seq_off, const uint8_t* reads2, uint32_t* coverage, uint32_t* support) {
    for (uint64_t i = 0; i < n_solid; ++i) if (spos[i] >= total_len || (i && spos[i - 1] >= spos[i])) return -1;
    for (uint32_t a = 0; a < n_reads; ++a) if (re[a] <= rb[a] || re[a] > total_len) return -1;
    Contig c(0, "votes", std::string((size_t)total_len, 'A'));
    VoteTables::set_solid(c, n_solid, spos, kids);
    for (uint32_t a = 0; a < n_reads; ++a) {
        Alignment al(rb[a], re[a], qae[a], reads2 + seq_off[a], nullptr, 0);
        al.update_solidkmers_support(k, c);
    }
    VoteTables::get_solid(c, coverage, support);
    return 0;
}

// Alignment::update_minimisers_support of every read, one Contig per contig of the tables (the arrays of HypoMegaWindows; a contig's
// length is its last border); rb / re are in the batch's coordinate space, read_contig names the contig.  OUT coverage / support
// [mw_off[n_info]].  -1: a read does not lie inside its contig.
int hypo_host_minimizer_votes(uint32_t n_contigs, const uint32_t* contig_base, const uint32_t* reg_base, const uint8_t* win_even, const uint32_t* info_base,
                              const uint32_t* start, uint32_t n_info, const uint32_t* mw_off, const uint32_t* rel_pos, const uint32_t* minimisers,
                              uint32_t n_reads, const uint32_t* rb, const uint32_t* re, const uint32_t* qae, const uint64_t* seq_off, const uint8_t* reads2,
                              const uint32_t* read_contig, uint32_t* coverage, uint32_t* support) {
    std::vector<std::unique_ptr<Contig>> ctg;
    for (uint32_t c = 0; c < n_contigs; ++c) {
        const uint32_t nb = reg_base[c + 1] - reg_base[c];
        const uint32_t len = nb ? start[reg_base[c + 1] - 1] : 0;
        const uint32_t x0 = info_base[c], x1 = c + 1 < n_contigs ? info_base[c + 1] : n_info;
        ctg.emplace_back(new Contig(c, "votes", std::string((size_t)len, 'A')));
        // (entry x of the contig is entry x0 + x of the tables: the offsets are taken relative to the contig's first entry)
        std::vector<uint32_t> off(mw_off + x0, mw_off + x1 + 1);
        const uint32_t e0 = off[0];
        for (uint32_t& o : off) o -= e0;
        VoteTables::set_mega(*ctg.back(), start + reg_base[c], nb, win_even[c] != 0, x1 - x0, off.data(), rel_pos + e0, minimisers + e0);
    }
    for (uint32_t a = 0; a < n_reads; ++a) {
        const uint32_t c = read_contig[a];
        if (c >= n_contigs || rb[a] < contig_base[c] || re[a] <= rb[a] || re[a] - contig_base[c] > ctg[c]->get_len()) return -1;
        Alignment al(rb[a] - contig_base[c], re[a] - contig_base[c], qae[a], reads2 + seq_off[a], nullptr, 0);
        al.update_minimisers_support(*ctg[c]);
    }
    for (uint32_t c = 0; c < n_contigs; ++c) {
        const uint32_t x0 = info_base[c], x1 = c + 1 < n_contigs ? info_base[c + 1] : n_info;
        std::vector<uint32_t> off(mw_off + x0, mw_off + x1 + 1);
        const uint32_t e0 = off[0];
        for (uint32_t& o : off) o -= e0;
        VoteTables::get_mega(*ctg[c], x1 - x0, off.data(), coverage + e0, support + e0);
    }
    return 0;
}

// The two host inline functions of edit_kernel.hpp that hypo_gpu_edit_scripts sizes the move storage of a wide pair with, as the
// device code compiles them (tests/test_edit_band_model_cpu.py holds tests/edit_band_model.py against them).
void hypo_host_edit_wide_band(uint32_t n, uint32_t m, uint32_t d, int64_t* lo, int64_t* hi) { hypo::edit_wide_band(n, m, d, *lo, *hi); }
uint64_t hypo_host_edit_wide_groups(int64_t lo, int64_t hi) { return hypo::edit_wide_groups(lo, hi); }

}  // extern "C"
