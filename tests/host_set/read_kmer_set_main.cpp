// read_kmer_set_main.cpp — host/ReadKmerSet.cpp and host/QvReport.cpp over plain host stand-ins for the device entry points they
// bind by name (tests/test_read_kmer_set_cpu.py builds this with -fsanitize=address,undefined -rdynamic and runs it).  The stand-ins
// keep the canonical k-mers in a map of 2-bit codes and follow include/hypo_gpu.h; what the classes are held against is computed here
// a second time from strings.  With -DHIDE_ONE_NAME the program lacks hypo_gpu_kset_size and only checks that bind() says so.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <sstream>
#include <string>
#include <unordered_map>
#include <vector>
#include "../../hypo_amd/csrc/host/QvReport.hpp"
#include "../../hypo_amd/csrc/host/ReadKmerSet.hpp"

namespace {
// ---- the stand-ins' state ----
struct Calls { int begin = 0, add = 0, size = 0, end = 0, enable = 0, spectrum = 0, min_count = 0, query = 0, track = 0; } g_calls;
std::unordered_map<uint64_t, uint8_t> g_set;               // canonical k-mer -> saturating count
uint32_t g_k = 0, g_t = 1, g_planes = 0, g_last_t = 0;
bool g_open = false, g_fail_begin = false;

int code(char c) {
    switch (c) { case 'A': case 'a': return 0; case 'C': case 'c': return 1; case 'G': case 'g': return 2; case 'T': case 't': return 3; default: return -1; }
}
// f(canonical k-mer) for every length-k window of bases in s[0, n), with the window's start
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
bool lacks(uint64_t key) { auto it = g_set.find(key); return it == g_set.end() || it->second < g_t; }
}  // namespace

extern "C" {
int hypo_gpu_kset_begin(uint32_t k, uint64_t, uint64_t) {
    ++g_calls.begin;
    if (g_fail_begin || k < 12 || k > 31) return HYPO_E_INVALID;
    g_set.clear(); g_k = k; g_t = 1; g_planes = 0; g_open = true;
    return HYPO_OK;
}
int hypo_gpu_kset_add(const char* bytes, uint64_t n) {
    ++g_calls.add;
    if (!g_open) return HYPO_E_INVALID;
    windows(bytes, n, [](uint64_t key, uint64_t) { uint8_t& c = g_set[key]; if (c < 255 && (g_planes || !c)) ++c; });
    return HYPO_OK;
}
#ifndef HIDE_ONE_NAME
int hypo_gpu_kset_size(uint64_t* n_distinct, uint64_t* table_bytes) {
    ++g_calls.size;
    if (!g_open) return HYPO_E_INVALID;
    if (n_distinct) *n_distinct = g_set.size();
    if (table_bytes) *table_bytes = 8 * g_set.size();
    return HYPO_OK;
}
#endif
int hypo_gpu_kset_end(void) { ++g_calls.end; g_open = false; g_set.clear(); return HYPO_OK; }
int hypo_gpu_kset_counts_enable(uint32_t n_texts) {
    ++g_calls.enable;
    if (!g_open || !g_set.empty() || g_planes || n_texts < 1 || n_texts > HYPO_KSET_MAX_TEXTS) return HYPO_E_INVALID;
    g_planes = n_texts;
    return HYPO_OK;
}
int hypo_gpu_kset_spectrum(uint32_t text, uint64_t* hist) {
    ++g_calls.spectrum;
    if (!g_open || text >= g_planes || !hist) return HYPO_E_INVALID;
    std::fill(hist, hist + HYPO_KSET_SPECTRUM_BINS, 0);
    for (const auto& kv : g_set) ++hist[(size_t)kv.second * 5];           // (nothing is ever marked here: column 0)
    return HYPO_OK;
}
int hypo_gpu_kset_min_count(uint32_t t) {
    ++g_calls.min_count;
    if (!g_open || !g_planes || t < 1 || t > 255) return HYPO_E_INVALID;
    g_t = g_last_t = t;
    return HYPO_OK;
}
int hypo_gpu_kset_query(const char* bytes, const uint64_t* off, uint32_t n_seqs, uint64_t* total, uint64_t* missing) {
    ++g_calls.query;
    if (!g_open) return HYPO_E_INVALID;
    for (uint32_t s = 0; s < n_seqs; ++s) {
        total[s] = missing[s] = 0;
        windows(bytes + off[s], off[s + 1] - off[s], [&](uint64_t key, uint64_t) { ++total[s]; missing[s] += lacks(key); });
    }
    return HYPO_OK;
}
// kset_kernel.hip, "where the missing windows are": a base is covered when a missing window contains it; an interval starts at a
// covered base whose predecessor is not covered (or which begins the sequence) and ends where the cover does
int hypo_gpu_kset_query_track(const char* bytes, const uint64_t* off, uint32_t n_seqs, const uint8_t* want, uint64_t* total, uint64_t* missing, uint64_t* iv_off,
                              uint64_t* iv_start, uint64_t* iv_end, uint64_t* iv_missing, uint64_t iv_cap) {
    ++g_calls.track;
    if (!g_open) return HYPO_E_INVALID;
    std::vector<uint64_t> st, en, cnt;
    iv_off[0] = 0;
    for (uint32_t s = 0; s < n_seqs; ++s) {
        total[s] = missing[s] = 0;
        const bool wanted = !want || want[s];
        windows(bytes + off[s], off[s + 1] - off[s], [&](uint64_t key, uint64_t at) {
            ++total[s];
            if (!lacks(key)) return;
            ++missing[s];
            if (!wanted) return;
            if (!st.empty() && st.size() > iv_off[s] && at <= en.back()) { en.back() = at + g_k; ++cnt.back(); }
            else { st.push_back(at); en.push_back(at + g_k); cnt.push_back(1); }
        });
        iv_off[s + 1] = st.size();
    }
    if (st.size() > iv_cap) return HYPO_E_WORKSPACE;
    std::copy(st.begin(), st.end(), iv_start); std::copy(en.begin(), en.end(), iv_end); std::copy(cnt.begin(), cnt.end(), iv_missing);
    return HYPO_OK;
}
}  // extern "C"

namespace {
int g_failed = 0;
#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); ++g_failed; } } while (0)

// ---- the second computation, on strings ----
uint64_t g_rng = 0x9E3779B97F4A7C15ull;
std::string random_bases(size_t n) {
    std::string s(n, 'A');
    for (char& c : s) { g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull; c = "ACGT"[g_rng >> 62]; }
    return s;
}
std::string canonical(const std::string& w) {
    std::string r(w.rbegin(), w.rend());
    for (char& c : r) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A';
    return std::min(w, r);
}
std::map<std::string, unsigned> naive_counts(const std::vector<std::string>& reads, size_t k) {
    std::map<std::string, unsigned> m;
    for (const std::string& r : reads)
        for (size_t i = 0; i + k <= r.size(); ++i) ++m[canonical(r.substr(i, k))];
    return m;
}
// the track's lines for one contig: the maximal runs of bases that a window missing from `have` contains
std::string naive_track(const std::string& name, const std::string& text, const std::map<std::string, unsigned>& have, size_t k, uint64_t& n_missing) {
    std::vector<char> miss(text.size() + 1, 0), covered(text.size() + 1, 0);
    for (size_t i = 0; i + k <= text.size(); ++i)
        if (!have.count(canonical(text.substr(i, k)))) { miss[i] = 1; std::fill(covered.begin() + (ptrdiff_t)i, covered.begin() + (ptrdiff_t)(i + k), 1); }
    std::ostringstream os;
    os << "#contig\tstart\tend\tmissing_kmers\n";
    n_missing = 0;
    for (size_t i = 0; i < text.size();) {
        if (!covered[i]) { ++i; continue; }
        size_t e = i, m = 0;
        while (covered[e]) { m += miss[e]; ++e; }
        os << name << '\t' << i << '\t' << e << '\t' << m << '\n';
        n_missing += m;
        i = e;
    }
    return os.str();
}

void lifecycle() {
    const uint32_t k = 21;
    const std::vector<std::string> reads = {random_bases(40), random_bases(33), random_bases(57)};
    hypo::ReadKmerSet set;
    CHECK(set.bind() && set.have_set() && !set.open());
    CHECK(set.begin(k, 1000, 0) == HYPO_OK && set.open() && set.k() == k);
    hypo::ReadSink sink = set.sink();
    CHECK(sink.k == k && !sink.exact);
    for (const std::string& r : reads) CHECK(sink.add(r.data(), r.size()) == HYPO_OK);
    CHECK(sink.add(reads[0].data(), reads[0].size()) == HYPO_OK);             // (a read seen twice: no new k-mer)
    CHECK(set.reads_done() == HYPO_OK && g_calls.size == 1);
    CHECK(set.n_distinct() == naive_counts(reads, k).size() && set.n_distinct() > 0);
    CHECK(set.min_count() == 1);
    set.end(); set.end();
    CHECK(g_calls.end == 1 && !set.open());
    // a begin that fails leaves nothing to end
    g_fail_begin = true;
    hypo::ReadKmerSet bad;
    CHECK(bad.bind() && bad.begin(k, 1000, 0) == HYPO_E_INVALID && !bad.open());
    bad.end();
    CHECK(g_calls.end == 1);
    g_fail_begin = false;
}

void min_count() {
    // k-mers seen once, twice, three and four times: 20, 25, 10 and 20 of them, so the histogram stops falling at 3
    const uint32_t k = 21;
    const std::string a = random_bases(40), b = random_bases(45), c = random_bases(30), d = random_bases(40);
    const std::vector<std::string> reads = {a, b, b, c, c, c, d, d, d, d};
    uint64_t h[hypo::ReadKmerSet::kRows] = {};
    for (const auto& kv : naive_counts(reads, k)) ++h[std::min(kv.second, 255u)];
    CHECK(h[1] == 20 && h[2] == 25 && h[3] == 10 && h[4] == 20);
    uint32_t valley = 2;
    for (uint32_t x = 2; x < 255; ++x) if (h[x] <= h[x + 1]) { valley = x; break; }
    CHECK(valley == 3 && hypo::ReadKmerSet::valley(h) == 3);
    hypo::ReadKmerSet set;
    CHECK(set.bind() && set.bind_counts() && set.have_counts() && set.have_min_count());
    CHECK(set.begin(k, 1000, 0) == HYPO_OK);
    const int enables = g_calls.enable;
    CHECK(set.enable_counts(1) == HYPO_OK && g_calls.enable == enables + 1 && g_planes == 1);
    hypo::ReadSink sink = set.sink();
    for (const std::string& r : reads) CHECK(sink.add(r.data(), r.size()) == HYPO_OK);
    CHECK(set.reads_done() == HYPO_OK && set.n_distinct() == 75);
    int calls = g_calls.min_count;
    CHECK(set.set_min_count(2) == HYPO_OK && set.min_count() == 2 && set.n_reliable() == h[2] + h[3] + h[4]);
    CHECK(g_calls.min_count == calls + 1 && g_last_t == 2);
    CHECK(set.set_min_count(0) == HYPO_OK && set.min_count() == valley && set.n_reliable() == h[3] + h[4]);
    CHECK(g_calls.min_count == calls + 2 && g_last_t == valley);
    set.end();
}

// `n_errors` single-base errors 45 bases apart in 54 000 bases at k = 21: every error is an interval of its own (41 bases, 21 windows)
void track(size_t n_errors, int want_calls) {
    const uint32_t k = 21;
    const std::string genome = random_bases(54000);
    std::string text = genome;
    for (size_t i = 0; i < n_errors; ++i) { char& c = text[20 + 45 * i]; c = c == 'A' ? 'C' : 'A'; }
    hypo::ReadKmerSet set;
    CHECK(set.bind() && set.bind_track() && set.have_track());
    CHECK(set.begin(k, 100000, 0) == HYPO_OK);
    CHECK(set.sink().add(genome.data(), genome.size()) == HYPO_OK && set.reads_done() == HYPO_OK);
    hypo::QvReport qv(set);
    CHECK(qv.bind());
    qv.keep_track();
    const int before = g_calls.track, queries = g_calls.query;
    CHECK(qv.push(0, genome, text) == HYPO_OK && qv.flush() == HYPO_OK);
    CHECK(g_calls.track == before + want_calls && g_calls.query == queries);
    uint64_t n_missing = 0;
    const std::string want = naive_track("ctg", text, naive_counts({genome}, k), k, n_missing);
    std::ostringstream got, table;
    qv.write_track(got, {"ctg"});
    CHECK(got.str() == want);
    CHECK((size_t)std::count(want.begin(), want.end(), '\n') == 1 + n_errors && n_missing == 21 * n_errors);
    const hypo::QvReport::TrackSums ts = qv.track_sums();
    CHECK(ts.intervals == n_errors && ts.bases == 41 * n_errors && ts.missing == n_missing);
    qv.write(table, {"ctg"});
    const std::string nw = std::to_string(genome.size() - k + 1);
    CHECK(table.str().find("ctg\t0\t" + nw + "\tinf\t" + std::to_string(n_missing) + "\t" + nw + "\t") != std::string::npos);
    set.end();
}
}  // namespace

int main() {
#ifdef HIDE_ONE_NAME
    hypo::ReadKmerSet set;
    CHECK(!set.bind() && !set.have_set());
#else
    lifecycle();
    min_count();
    track(1200, 2);          // more intervals than the first call's room, 1024 + 108 000 / 1024
    track(10, 1);
#endif
    if (g_failed) return 1;
    std::puts("read_kmer_set: ok");
    return 0;
}
