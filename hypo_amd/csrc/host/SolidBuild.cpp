// SolidBuild.cpp — see SolidBuild.hpp.
#include "SolidBuild.hpp"
#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <dlfcn.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>
#include "SeqIO.hpp"

namespace hypo {

// Literal restatement of suk::SolidKmers::find_cutoffs (SolidKmers.cpp:258-363).  UINT is 32 bits there and histArray holds size_t:
// the assignments and the arithmetic below keep those widths (global_maxima_val truncated on assignment, delta_sum wrapping, the
// quotient taken in 64 bits and truncated).  The only departure: where the reference would read delta_avg[bind] beyond the vector
// (bind == eind, no loop iteration follows, the value is never used) nothing is read.
bool find_cutoffs(const std::vector<uint64_t>& histArray, CutOffs& coffs) {
    typedef uint32_t UINT;
    coffs = CutOffs();
    const int len = (int)histArray.size() - 1;
    int ind = 2;
    while (ind < len && histArray[ind] > histArray[ind + 1]) ++ind;
    const int err_th = (ind > 100) ? 2 : ind;
    coffs.err = UINT(err_th);

    UINT global_maxima_val = 0;
    bool have_mean = false;
    for (ind = err_th + 1; ind < len; ++ind) {
        if (histArray[ind] > global_maxima_val) {
            global_maxima_val = (UINT)histArray[ind];
            coffs.mean = UINT(ind);
            have_mean = true;
        }
    }
    if (!have_mean) return false;

    const int cMax_lookup = 5;
    int bind = (int)coffs.mean - 1;
    int eind = err_th;
    coffs.lower = UINT(eind);
    UINT count_ge = 0, count_lower = 0;
    for (ind = bind; ind >= eind; --ind) {
        count_ge = 0; count_lower = 0;
        for (int ind2 = ind - 1; ind2 >= (ind - cMax_lookup) && ind2 >= eind; --ind2) {
            if (histArray[ind2] < histArray[ind]) ++count_lower;
            else ++count_ge;
        }
        if (count_ge >= count_lower) { coffs.lower = UINT(ind); break; }
    }

    bind = (int)coffs.mean + 1;
    eind = (int)std::min(UINT(bind) + 2 * (coffs.mean - coffs.lower), UINT(len));
    coffs.upper = UINT(eind);
    bool plan_a = false;
    for (ind = bind; ind < eind; ++ind) {
        count_lower = 0; count_ge = 0;
        for (UINT ind2 = ind + 1; ind2 <= UINT(ind + cMax_lookup) && ind2 < UINT(len); ++ind2) {
            if (histArray[ind2] < histArray[ind]) ++count_lower;
            else ++count_ge;
        }
        if (count_ge >= count_lower) { coffs.upper = UINT(ind); plan_a = true; break; }
    }
    if (!plan_a && bind < eind) {
        std::vector<UINT> delta_avg((size_t)eind, 0);
        for (ind = bind; ind < eind; ++ind) {
            UINT delta_sum = 0;
            count_lower = 0;
            for (int ind2 = ind + 1; ind2 <= ind + cMax_lookup && ind2 < len; ++ind2) {
                if (histArray[ind2] < histArray[ind]) {
                    ++count_lower;
                    delta_sum += (UINT)(histArray[ind] - histArray[ind2]);
                }
            }
            delta_avg[ind] = UINT((uint64_t)(UINT)(delta_sum * 100u) / ((uint64_t)count_lower * histArray[ind]));
        }
        float min_avg_avg_val = float(delta_avg[bind]);
        for (ind = bind; ind < eind; ++ind) {
            const UINT window_len = (UINT)std::min(cMax_lookup, eind - ind);
            UINT avg_delta_sum = 0;
            for (UINT ind2 = ind; ind2 < ind + window_len; ++ind2) avg_delta_sum += delta_avg[ind2];
            const float avg_avg_val = float(avg_delta_sum) / float(window_len);
            if (avg_avg_val < min_avg_avg_val) { min_avg_avg_val = avg_avg_val; coffs.upper = UINT(ind); }
        }
    }
    return true;
}

namespace {

// The ABI 9 entry points are bound by name when stage 0 runs, not at load time: the binary is linked with immediate binding, and a
// device library without them (the CPU stand-in of the tests, an ABI 8 build) must still serve every run that starts from stage 1.
struct KmerApi {
    int (*begin)(uint32_t, uint32_t) = nullptr;
    int (*add)(const char*, uint64_t) = nullptr;
    int (*histogram)(uint64_t*, uint32_t) = nullptr;
    int (*build)(uint32_t, uint32_t, int, uint64_t*, uint64_t*, uint64_t*) = nullptr;
    int (*end)(void) = nullptr;
    bool bind() {
        begin = (decltype(begin))dlsym(RTLD_DEFAULT, "hypo_gpu_kmer_count_begin");
        add = (decltype(add))dlsym(RTLD_DEFAULT, "hypo_gpu_kmer_count_add");
        histogram = (decltype(histogram))dlsym(RTLD_DEFAULT, "hypo_gpu_kmer_histogram");
        build = (decltype(build))dlsym(RTLD_DEFAULT, "hypo_gpu_solid_set_build");
        end = (decltype(end))dlsym(RTLD_DEFAULT, "hypo_gpu_kmer_count_end");
        return begin && add && histogram && build && end;
    }
};

// Sequence bytes of the read files, cut into chunks for hypo_gpu_kmer_count_add: the bases of a record (its sequence lines
// joined), one '\n' between records.  A chunk that fills up in the middle of a record is handed over as it is and the next chunk
// starts with its last k - 1 bytes: every k-mer lies whole in exactly one chunk.  (With a second consumer whose k-mers are longer,
// k is the larger of the two and next() says how many bytes at the front of a chunk are such a repeat: the count table, which must
// see every k-mer once, is given the chunk from its own k - 1 bytes before the end of that lead.)
class ChunkPipe {
public:
    ChunkPipe(size_t cap, uint32_t k) : _cap(cap), _carry(k - 1) {
        for (auto& b : _buf) {
            void* p = nullptr;
            if (hypo_gpu_host_alloc(cap, &p) == HYPO_OK) { b.data = (char*)p; b.pinned = true; }
            else { b.own.resize(cap); b.data = b.own.data(); }
        }
    }
    ~ChunkPipe() { for (auto& b : _buf) if (b.pinned) (void)hypo_gpu_host_free(b.data); }
    // producer side (the parser thread)
    void put(const char* p, size_t n) {
        while (n) {
            Buf& b = _buf[_fill];
            const size_t take = std::min(n, _cap - b.n);
            std::memcpy(b.data + b.n, p, take);
            b.n += take; p += take; n -= take;
            if (b.n == _cap) hand_over(true);
        }
    }
    void sep() { if (_buf[_fill].n && _buf[_fill].data[_buf[_fill].n - 1] != '\n') { const char c = '\n'; put(&c, 1); } }
    void finish() { if (_buf[_fill].n) hand_over(false); std::lock_guard<std::mutex> lk(_mu); _done = true; _cv.notify_all(); }
    // consumer side: the next full chunk (nullptr at the end); release() when it has been counted
    const char* next(size_t& n, size_t& lead) {
        std::unique_lock<std::mutex> lk(_mu);
        _cv.wait(lk, [this] { return _ready >= 0 || _done; });
        if (_ready < 0) return nullptr;
        _taking = _ready; _ready = -1;
        n = _buf[_taking].n;
        lead = _buf[_taking].lead;
        return _buf[_taking].data;
    }
    void release() { std::lock_guard<std::mutex> lk(_mu); _buf[_taking].n = 0; _taking = -1; _cv.notify_all(); }
    void abort() { std::lock_guard<std::mutex> lk(_mu); _aborted = true; _cv.notify_all(); }
    bool aborted() { std::lock_guard<std::mutex> lk(_mu); return _aborted; }
    uint64_t bytes_out = 0;
private:
    struct Buf { char* data = nullptr; size_t n = 0, lead = 0; bool pinned = false; std::vector<char> own; };
    void hand_over(bool carry) {
        std::unique_lock<std::mutex> lk(_mu);
        const int other = _fill ^ 1;
        _cv.wait(lk, [&] { return _aborted || (_ready < 0 && _taking != other && _buf[other].n == 0); });
        if (_aborted) { _buf[_fill].n = 0; return; }
        Buf& cur = _buf[_fill];
        Buf& nxt = _buf[other];
        bytes_out += cur.n;
        nxt.lead = 0;
        if (carry && _carry) { std::memcpy(nxt.data, cur.data + cur.n - _carry, _carry); nxt.n = nxt.lead = _carry; }
        _ready = _fill; _fill = other;
        _cv.notify_all();
    }
    size_t _cap, _carry;
    Buf _buf[2];
    int _fill = 0, _ready = -1, _taking = -1;
    bool _done = false, _aborted = false;
    std::mutex _mu; std::condition_variable _cv;
};

// one file into the pipe; false (and err) when its format is not FASTA or FASTQ
bool parse_reads(const std::string& path, ChunkPipe& pipe, uint64_t& file_bytes, std::string& err) {
    LineReader lr(path);
    if (!lr.ok()) { err = "cannot open " + path; return false; }
    std::string line;
    bool have = lr.next(line);
    while (have && line.empty()) { file_bytes += 1; have = lr.next(line); }
    if (!have) return true;                                              // an empty file holds no k-mers
    if (line[0] != '>' && line[0] != '@') { err = "cannot identify the format of " + path + " (neither FASTA nor FASTQ)"; return false; }
    const bool fq = line[0] == '@';
    while (have) {
        file_bytes += line.size() + 1;
        if (line.empty()) { have = lr.next(line); continue; }
        if (!fq) {
            if (line[0] == '>') pipe.sep();
            else pipe.put(line.data(), line.size());
            have = lr.next(line);
            continue;
        }
        if (line[0] != '@') { err = "malformed FASTQ record in " + path + " (a header line must start with '@')"; return false; }
        pipe.sep();
        size_t n_seq = 0;
        have = lr.next(line);
        while (have && !(line.size() && line[0] == '+')) { file_bytes += line.size() + 1; pipe.put(line.data(), line.size()); n_seq += line.size(); have = lr.next(line); }
        if (have) {                                                      // the '+' line, then as many quality characters as bases
            file_bytes += line.size() + 1;
            size_t q = 0;
            have = lr.next(line);
            while (have && q < n_seq) { file_bytes += line.size() + 1; q += line.size(); have = lr.next(line); }
        }
        if (pipe.aborted()) return true;
    }
    pipe.sep();
    return true;
}

double secs(std::chrono::steady_clock::time_point a) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - a).count(); }

// The files through one parser thread and the pipe; consume(chunk, n, lead) on the calling thread, false (with `err` set) to stop.
template <class Consume>
int pump_reads(const std::vector<std::string>& files, uint32_t k, SolidBuildStats& stats, std::string& err, Consume consume) {
    // HYPO_READ_CHUNK_KB: another chunk size (at least 4 KiB), so that a small read set comes in many chunks (tests/test_gpu_spectra.py)
    size_t chunk_bytes = (size_t)256 << 20;
    if (const char* kb = std::getenv("HYPO_READ_CHUNK_KB")) chunk_bytes = (size_t)std::max(4L, std::atol(kb)) << 10;
    int rc = SOLID_OK;
    ChunkPipe pipe(chunk_bytes, k);
    std::string perr;
    bool parse_ok = true;
    double parse_s = 0;
    std::thread parser([&] {
        const auto tp = std::chrono::steady_clock::now();
        for (const auto& f : files) if (!(parse_ok = parse_reads(f, pipe, stats.file_bytes, perr)) || pipe.aborted()) break;
        pipe.finish();
        parse_s = secs(tp);
    });
    size_t n = 0, lead = 0;
    while (const char* chunk = pipe.next(n, lead)) {
        if (rc == SOLID_OK && (rc = consume(chunk, n, lead)) != SOLID_OK) pipe.abort();
        pipe.release();
    }
    parser.join();
    stats.parse_s = parse_s;
    stats.seq_bytes = pipe.bytes_out;
    if (rc == SOLID_OK && !parse_ok) { err = perr; rc = SOLID_E_INPUT; }
    return rc;
}

// one chunk into the second consumer; lead: the bytes at its start that the chunk before it held already
int sink_chunk(ReadSink& sink, const char* chunk, size_t n, size_t lead, SolidBuildStats& stats, std::string& err) {
    const size_t skip = sink.exact && lead > sink.k - 1 ? lead - (sink.k - 1) : 0;
    const auto tc = std::chrono::steady_clock::now();
    const int rc = sink.add(chunk + skip, n - skip);
    stats.sink_s += secs(tc);
    if (rc == HYPO_OK) return SOLID_OK;
    err = hypo_gpu_last_error();
    return SOLID_E_SINK;
}

}  // namespace

int stream_reads(const std::vector<std::string>& files, ReadSink& sink, SolidBuildStats& stats, std::string& err) {
    const auto t0 = std::chrono::steady_clock::now();
    stats = SolidBuildStats();
    if (files.empty()) { err = "no read files"; return SOLID_E_INPUT; }
    const int rc = pump_reads(files, sink.k, stats, err, [&](const char* chunk, size_t n, size_t lead) { return sink_chunk(sink, chunk, n, lead, stats, err); });
    stats.total_s = secs(t0);
    return rc;
}

int build_solid_kmers(const std::vector<std::string>& files, uint32_t k, uint32_t coverage, int threads, SolidKmers& sk,
                      SolidBuildStats& stats, std::string& err, ReadSink* sink) {
    (void)threads;                               // one parser thread and the thread that drives the device
    const auto t0 = std::chrono::steady_clock::now();
    stats = SolidBuildStats();
    if (k < 5 || k > 17) {
        char b[256];
        std::snprintf(b, sizeof b, "k = %u is not supported by the device construction (5..17): the set alone needs 4^k bits = %.1f GiB, "
                                   "the count table 4^k counters = %.0f GiB", k, k < 32 ? (double)(1ull << (2 * k)) / 8 / (1u << 30) : 0.0,
                      k < 32 ? (double)(1ull << (2 * k)) / (1u << 30) : 0.0);
        err = b;
        return SOLID_E_K;
    }
    if (files.empty()) { err = "no read files"; return SOLID_E_INPUT; }
    KmerApi api;
    if (!api.bind()) { err = "the device library does not provide the k-mer counting entry points (hypo_gpu_kmer_*, ABI 9)"; return SOLID_E_DEVICE; }
    if (api.begin(k, coverage) != HYPO_OK) { err = hypo_gpu_last_error(); return SOLID_E_DEVICE; }
    struct End { KmerApi& a; ~End() { (void)a.end(); } } end_table{api};      // the table is freed on every way out
    // (the chunks overlap by the longer of the two k-mers less one; the count table gets each from its own k - 1 bytes before the new
    // ones, and so does a sink that counts)
    const int rc = pump_reads(files, sink ? std::max(k, sink->k) : k, stats, err, [&](const char* chunk, size_t n, size_t lead) {
        const size_t skip = lead > k - 1 ? lead - (k - 1) : 0;
        const auto tc = std::chrono::steady_clock::now();
        const int arc = api.add(chunk + skip, n - skip);
        stats.count_s += secs(tc);
        if (arc != HYPO_OK) { err = hypo_gpu_last_error(); return (int)SOLID_E_DEVICE; }
        return sink ? sink_chunk(*sink, chunk, n, lead, stats, err) : (int)SOLID_OK;
    });
    if (rc != SOLID_OK) return rc;
    auto th = std::chrono::steady_clock::now();
    stats.hist.assign((size_t)4 * coverage + 1, 0);
    if (api.histogram(stats.hist.data(), (uint32_t)stats.hist.size()) != HYPO_OK) { err = hypo_gpu_last_error(); return SOLID_E_DEVICE; }
    stats.hist_s = secs(th);
    if (!find_cutoffs(stats.hist, stats.cut)) { err = "the k-mer histogram has no maximum after the error threshold"; return SOLID_E_UNDEFINED; }
    std::fprintf(stdout, "[SolidKmers] Info: Error-threshold freq: %u, Lower-threshold freq: %u, Upper-threshold freq: %u, Mean-coverage: %u\n",
                 stats.cut.err, stats.cut.lower, stats.cut.upper, stats.cut.mean);
    th = std::chrono::steady_clock::now();
    sk.k = k;
    sk.words.assign((size_t)((1ull << (2 * k)) / 64), 0);
    if (api.build(stats.cut.lower, stats.cut.upper, 1, sk.words.data(), &stats.n_bits, &stats.n_canonical) != HYPO_OK) {
        err = hypo_gpu_last_error(); return SOLID_E_DEVICE;
    }
    stats.fill_s = secs(th);
    sk.num_solid = stats.n_canonical;
    std::fprintf(stdout, "[SolidKmers] Info: Number of solid kmers found: %lu\n", (unsigned long)stats.n_bits);
    stats.total_s = secs(t0);
    return SOLID_OK;
}

}  // namespace hypo
