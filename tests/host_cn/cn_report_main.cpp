// cn_report_main.cpp — host/CnReport.cpp and ReadKmerSet::query_depth / peak over plain host stand-ins for the device entry points
// they bind by name (tests/test_cn_report_cpu.py builds this with -fsanitize=address,undefined -rdynamic and runs it).  The stand-ins
// keep the read counts and the copy numbers in maps of 2-bit codes and follow include/hypo_gpu.h.  Checked here: a text cut into
// calls at contig ends, and one long contig cut at multiples of the bin with k - 1 bytes of overlap, give the arrays of one call; no
// call is larger than asked; the text is marked once, whole, before the first depth call, or not at all when another flag has
// marked it; the file lists the contigs in draft order whatever order they were written in; a histogram without a peak is reported.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <sstream>
#include <string>
#include <unordered_map>
#include <vector>
#include "../../hypo_amd/csrc/host/CnReport.hpp"
#include "../../hypo_amd/csrc/host/ReadKmerSet.hpp"

namespace {
std::unordered_map<uint64_t, uint32_t> g_reads, g_text[2];     // canonical k-mer -> count (saturated where it is read)
uint32_t g_k = 0, g_t = 1;
struct Calls { int mark = 0, depth = 0, spectrum = 0; uint64_t largest = 0, marked_bytes = 0; bool mark_after_depth = false; } g_calls;

int code(char c) {
    switch (c) { case 'A': case 'a': return 0; case 'C': case 'c': return 1; case 'G': case 'g': return 2; case 'T': case 't': return 3; default: return -1; }
}
template <class F> void windows(const char* s, uint64_t n, F f) {
    const uint64_t mask = (1ull << (2 * g_k)) - 1;
    uint64_t fw = 0, rc = 0, run = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const int c = code(s[i]);
        if (c < 0) { run = 0; continue; }
        fw = ((fw << 2) | (uint64_t)c) & mask;
        rc = (rc >> 2) | ((uint64_t)(3 - c) << (2 * (g_k - 1)));
        if (++run >= g_k) f(std::min(fw, rc), i + 1 - g_k);
    }
}
uint32_t sat(const std::unordered_map<uint64_t, uint32_t>& m, uint64_t key) { auto it = m.find(key); return it == m.end() ? 0 : std::min(it->second, 255u); }

struct Bin { uint32_t windows = 0, missing = 0, rated = 0, over = 0, under = 0, median = 0; std::vector<uint32_t> cs; };
// the definition of include/hypo_gpu.h for one sequence, bin by bin
std::vector<Bin> bins_of(const char* s, uint64_t len, uint32_t bin, uint32_t plane, uint32_t unit) {
    std::vector<Bin> out((len + bin - 1) / bin);
    windows(s, len, [&](uint64_t key, uint64_t start) {
        Bin& b = out[start / bin];
        ++b.windows;
        const uint32_t c = sat(g_reads, key), m = sat(g_text[plane], key);
        if (c < g_t) { ++b.missing; return; }
        b.cs.push_back(c);
        if (m >= 1 && m <= 254 && c <= 254) { ++b.rated; if (2 * c >= 3 * unit * m) ++b.over; if (4 * c <= 3 * unit * m) ++b.under; }
    });
    for (Bin& b : out) { std::sort(b.cs.begin(), b.cs.end()); b.median = b.cs.empty() ? 0 : b.cs[(b.cs.size() + 1) / 2 - 1]; }
    return out;
}
#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "cn_report: line %d: %s\n", __LINE__, #x); std::exit(1); } } while (0)
}  // namespace

extern "C" {
int hypo_gpu_kset_begin(uint32_t k, uint64_t, uint64_t) { g_k = k; return HYPO_OK; }
int hypo_gpu_kset_add(const char* bytes, uint64_t n) { windows(bytes, n, [](uint64_t key, uint64_t) { ++g_reads[key]; }); return HYPO_OK; }
int hypo_gpu_kset_size(uint64_t* n, uint64_t*) { if (n) *n = g_reads.size(); return HYPO_OK; }
int hypo_gpu_kset_end(void) { return HYPO_OK; }
int hypo_gpu_kset_counts_enable(uint32_t) { return HYPO_OK; }
int hypo_gpu_kset_min_count(uint32_t t) { g_t = t; return HYPO_OK; }
int hypo_gpu_kset_spectrum(uint32_t text, uint64_t* hist) {
    ++g_calls.spectrum;
    for (int i = 0; i < HYPO_KSET_SPECTRUM_BINS; ++i) hist[i] = 0;
    for (const auto& kv : g_reads) ++hist[(size_t)std::min(kv.second, 255u) * 5 + std::min(sat(g_text[text], kv.first), 4u)];
    return HYPO_OK;
}
int hypo_gpu_kset_mark(uint32_t text, const char* bytes, const uint64_t* off, uint32_t n_seqs, uint64_t*, uint64_t*) {
    ++g_calls.mark;
    if (g_calls.depth) g_calls.mark_after_depth = true;
    for (uint32_t s = 0; s < n_seqs; ++s) {
        g_calls.marked_bytes += off[s + 1] - off[s];
        windows(bytes + off[s], off[s + 1] - off[s], [&](uint64_t key, uint64_t) { if (g_reads.count(key)) ++g_text[text][key]; });
    }
    return HYPO_OK;
}
int hypo_gpu_kset_query_depth(const char* bytes, const uint64_t* off, uint32_t n_seqs, uint32_t bin, uint32_t text, uint32_t unit, uint64_t n_bins,
                              uint32_t* windows_, uint32_t* missing, uint32_t* rated, uint32_t* over, uint32_t* under, uint8_t* med_count) {
    ++g_calls.depth;
    if (bin < HYPO_KSET_DEPTH_MIN_BIN || bin > HYPO_KSET_DEPTH_MAX_BIN || unit < 1 || unit > 255 || text > 1) return HYPO_E_INVALID;
    uint64_t want = 0;
    for (uint32_t s = 0; s < n_seqs; ++s) want += (off[s + 1] - off[s] + bin - 1) / bin;
    if (want != n_bins) return HYPO_E_INVALID;
    if (n_seqs) g_calls.largest = std::max<uint64_t>(g_calls.largest, off[n_seqs] - off[0]);
    uint64_t b = 0;
    for (uint32_t s = 0; s < n_seqs; ++s)
        for (const Bin& x : bins_of(bytes + off[s], off[s + 1] - off[s], bin, text, unit)) {
            windows_[b] = x.windows; missing[b] = x.missing; rated[b] = x.rated; over[b] = x.over; under[b] = x.under; med_count[b] = (uint8_t)x.median;
            ++b;
        }
    return HYPO_OK;
}
}

int main() {
    using namespace hypo;
    std::mt19937 rng(77);
    auto rnd = [&](size_t n) { std::string s(n, 'A'); for (char& c : s) c = "ACGT"[rng() % 4]; return s; };
    // the peak of a histogram
    {
        uint64_t h[256] = {0};
        CHECK(ReadKmerSet::peak(h) == 0);
        h[1] = 100; h[2] = 50; h[3] = 20; h[4] = 30; h[5] = 60; h[6] = 60; h[7] = 10;
        CHECK(ReadKmerSet::valley(h) == 3 && ReadKmerSet::peak(h) == 5);
        uint64_t g[256] = {0};
        g[255] = 1000; g[1] = 500; g[2] = 3;
        CHECK(ReadKmerSet::peak(g) == 0);
        g[254] = 1;
        CHECK(ReadKmerSet::peak(g) == 254);
    }
    ReadKmerSet set;
    CHECK(set.bind() && set.bind_counts() && set.bind_depth() && set.have_depth());
    const uint32_t k = 21;
    CHECK(set.begin(k, 0, 0) == HYPO_OK);
    // five contigs: a repeat read at twice the depth and collapsed in the text, one stretch the text has twice, Ns, a short one, an empty one
    const std::string genome = rnd(9000);
    std::vector<std::string> contigs = {genome.substr(0, 3000), "", genome.substr(3000, 10), genome.substr(3000, 4000) + "NNNN" + genome.substr(6000, 600), genome.substr(7000, 2000)};
    ReadSink sink = set.sink();
    for (int d = 0; d < 12; ++d) CHECK(sink.add(genome.data(), genome.size()) == HYPO_OK);
    for (int d = 0; d < 12; ++d) CHECK(sink.add(genome.data() + 500, 700) == HYPO_OK);            // read 24 times, once in the text
    CHECK(set.reads_done() == HYPO_OK);
    const std::vector<std::string> names = {"c0", "c1", "c2", "c3", "c4"};
    const std::vector<size_t> order = {0, 1, 3, 2, 4};                                              // (written in another order than the draft's)
    for (int own = 1; own >= 0; --own) {
        g_calls = Calls(); g_text[0].clear(); g_text[1].clear();
        const uint32_t plane = own ? 0 : 1, bin = 100;
        if (!own) {                                                                                 // another flag has marked plane 1
            for (const std::string& c : contigs) { const uint64_t o[2] = {0, c.size()}; hypo_gpu_kset_mark(1, c.data(), o, 1, nullptr, nullptr); }
            g_calls = Calls();
        }
        CnReport cn(set);
        CHECK(cn.bind());
        cn.configure(bin, 0, plane, own != 0);
        size_t total = 0;
        for (size_t c : order) { cn.push(c, contigs[c]); total += contigs[c].size(); }
        const char* what = "";
        CHECK(cn.run(what) == HYPO_OK);
        CHECK(g_calls.mark == (own ? 1 : 0) && !g_calls.mark_after_depth && g_calls.marked_bytes == (own ? total : 0));
        CHECK(cn.unit() == 12 && !cn.unit_given() && cn.bin() == bin && cn.k() == k);
        std::ostringstream got, want;
        cn.write(got, names);
        want << "##hypo-qv-cn\tk=21\tbin=100\tunit=12\tpeak\tmin_count=1\n#contig\tstart\tend\twindows\tmissing\trated\tover\tunder\tmedian_count\tcall\n";
        CnReport::Sums sums;
        for (size_t c = 0; c < contigs.size(); ++c) {
            const std::vector<Bin> bs = bins_of(contigs[c].data(), contigs[c].size(), bin, plane, 12);
            for (size_t j = 0; j < bs.size(); ++j) {
                const Bin& b = bs[j];
                const uint64_t end = std::min<uint64_t>((j + 1) * bin, contigs[c].size());
                const char* call = 2 * b.over > b.rated ? "collapsed" : 2 * b.under > b.rated ? "duplicated" : ".";
                want << names[c] << '\t' << j * bin << '\t' << end << '\t' << b.windows << '\t' << b.missing << '\t' << b.rated << '\t' << b.over << '\t' << b.under << '\t'
                     << b.median << '\t' << call << '\n';
                ++sums.bins;
                if (call[0] == 'c') { ++sums.collapsed; sums.collapsed_bases += end - j * bin; }
                if (call[0] == 'd') { ++sums.duplicated; sums.duplicated_bases += end - j * bin; }
            }
        }
        CHECK(got.str() == want.str());
        const CnReport::Sums s = cn.sums();
        CHECK(s.bins == sums.bins && s.collapsed == sums.collapsed && s.collapsed_bases == sums.collapsed_bases && s.duplicated == sums.duplicated &&
              s.duplicated_bases == sums.duplicated_bases);
        CHECK(s.collapsed >= 5 && s.duplicated >= 5 && s.bins == 30 + 1 + 47 + 20);               // the repeat, and the 600 bases c3 has twice
    }
    // the text in calls: whatever the bound on a call, the arrays are those of one call, and no call is larger than the bound
    {
        std::string text;
        std::vector<uint64_t> off{0};
        for (const std::string& c : contigs) { text += c; off.push_back(text.size()); }
        for (uint32_t bin : {32u, 100u, 1024u}) {
            ReadKmerSet::Depth one;
            g_calls = Calls();
            CHECK(set.query_depth(text, off, bin, 0, 12, one) == HYPO_OK && g_calls.depth == 1);
            CHECK(one.windows.size() == (3000 + bin - 1) / bin + 1 + (4604 + bin - 1) / bin + (2000 + bin - 1) / bin);
            for (size_t per_call : {(size_t)bin + k, (size_t)1500, (size_t)2100, (size_t)3000, (size_t)4604, (size_t)7000}) {
                ReadKmerSet::Depth cut;
                g_calls = Calls();
                CHECK(set.query_depth(text, off, bin, 0, 12, cut, per_call) == HYPO_OK);
                CHECK(g_calls.depth > 1 && g_calls.largest <= per_call);
                CHECK(cut.windows == one.windows && cut.missing == one.missing && cut.rated == one.rated && cut.over == one.over && cut.under == one.under && cut.median == one.median);
            }
        }
    }
    // a least count, a given unit, and a histogram without a peak
    {
        g_calls = Calls(); g_text[0].clear();
        CHECK(set.set_min_count(13) == HYPO_OK);
        CnReport cn(set);
        CHECK(cn.bind());
        cn.configure(64, 7, 0, true);
        cn.push(0, contigs[0]);
        const char* what = "";
        CHECK(cn.run(what) == HYPO_OK && cn.unit() == 7 && cn.unit_given() && g_calls.spectrum == 1);   // (the one of set_min_count)
        std::ostringstream got;
        cn.write(got, names);
        CHECK(got.str().rfind("##hypo-qv-cn\tk=21\tbin=64\tunit=7\tgiven\tmin_count=13\n", 0) == 0);
        CHECK(cn.sums().bins == 47);
        g_reads.clear(); g_text[0].clear();
        g_reads[5] = 300;                                                                          // every k-mer at the cap: no peak
        CnReport none(set);
        CHECK(none.bind());
        none.configure(64, 0, 0, true);
        none.push(0, contigs[0]);
        CHECK(none.run(what) == CnReport::E_NO_PEAK);
    }
    set.end();
    std::printf("cn_report: ok\n");
    return 0;
}
