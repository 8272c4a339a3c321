// capi.hip — the C-ABI of include/hypo_gpu.h on top of the gfx950 kernels.
// No CPU implementation of the hot path exists in this library: without a HIP device every entry
// point fails with HYPO_E_NODEVICE / HYPO_E_NOTINIT.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <dlfcn.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>
#include "../../include/hypo_gpu.h"
#include "poa_kernel.hpp"
#include "arms_kernel.hpp"
#include "support_kernel.hpp"
#include "scan_kernel.hpp"
#include "kmer_kernel.hpp"
#include "edit_kernel.hpp"
#include "kset_kernel.hpp"

namespace {

thread_local char tl_err[512] = "";
thread_local HypoPoaStats tl_stats;

int fail(int code, const char* fmt, ...) {
    va_list ap; va_start(ap, fmt); vsnprintf(tl_err, sizeof(tl_err), fmt, ap); va_end(ap);
    return code;
}
#define HIP_TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(HYPO_E_HIP, "%s: %s", #x, hipGetErrorString(e_)); } while (0)

// ---- host -> device copies of the host-pointer entry points ---------------------------------------------------------------
// A caller of the C-ABI hands over ordinary (pageable) memory: the reference's objects know nothing of page-locked buffers, and
// locking a few GB for one upload costs more than the upload (MI355X box, profiles/history/r04_pin_bench.txt: hipHostMalloc 0.18 s per GB
// + 0.12 s per GB to free it; a copy out of page-locked memory 57 GB/s, out of pageable memory 15-25 GB/s).  Large copies out of
// pageable memory are therefore staged here: a few threads copy the next 32 MB into one of two page-locked bounce buffers of the
// context while the DMA engine drains the other.  Memory the caller did page-lock (hypo_gpu_host_alloc) is copied from directly.
class CopyPool {                                   // a handful of threads that memcpy slices side by side (one pool per process)
public:
    void copy(char* d, const char* s, size_t n) {
        constexpr size_t kSlice = (size_t)2 << 20;
        if (n <= kSlice) { memcpy(d, s, n); return; }
        std::unique_lock<std::mutex> lk(mu);
        if (th.empty()) for (int i = 0; i < kWorkers; ++i) th.emplace_back([this] { work(); });
        for (size_t at = 0; at < n; at += kSlice) jobs.push_back(Job{d + at, s + at, n - at < kSlice ? n - at : kSlice});
        left += jobs.size() - next;
        cv.notify_all();
        while (next < jobs.size()) {                 // the caller takes slices too
            const Job j = jobs[next++];
            lk.unlock(); memcpy(j.d, j.s, j.n); lk.lock();
            --left;
        }
        done.wait(lk, [this] { return left == 0; });
        jobs.clear(); next = 0;
    }
    ~CopyPool() { { std::lock_guard<std::mutex> lk(mu); quit = true; } cv.notify_all(); for (auto& t : th) t.join(); }
private:
    static constexpr int kWorkers = 7;          // (+ the caller; 16 threads were no faster: 13-21 GB/s next to the parser threads of the next batch)
    struct Job { char* d; const char* s; size_t n; };
    std::vector<std::thread> th; std::vector<Job> jobs; size_t next = 0, left = 0; bool quit = false;
    std::mutex mu; std::condition_variable cv, done;
    void work() {
        std::unique_lock<std::mutex> lk(mu);
        for (;;) {
            cv.wait(lk, [this] { return quit || next < jobs.size(); });
            if (quit) return;
            const Job j = jobs[next++];
            lk.unlock(); memcpy(j.d, j.s, j.n); lk.lock();
            if (--left == 0) done.notify_all();
        }
    }
};
CopyPool g_copy_pool;
std::mutex g_copy_mu;                              // one staged copy at a time uses the pool

struct Bounce {
    static constexpr size_t kChunk = (size_t)32 << 20;
    void* buf[2] = {nullptr, nullptr}; hipEvent_t ev[2] = {nullptr, nullptr}; bool used[2] = {false, false}; int turn = 0;
    hipError_t ensure() {
        if (buf[0]) return hipSuccess;
        for (int i = 0; i < 2; ++i) {
            hipError_t e = hipHostMalloc(&buf[i], kChunk, hipHostMallocNonCoherent);
            if (e != hipSuccess) return e;
            if ((e = hipEventCreateWithFlags(&ev[i], hipEventDisableTiming)) != hipSuccess) return e;
        }
        return hipSuccess;
    }
    void release() { for (int i = 0; i < 2; ++i) { if (ev[i]) (void)hipEventDestroy(ev[i]); if (buf[i]) (void)hipHostFree(buf[i]); buf[i] = nullptr; ev[i] = nullptr; used[i] = false; } }
};

// Device buffers of the host-pointer entry points: grow-only arenas owned by the context (no allocation in the
// steady-state path); released at shutdown.  Slot numbers are local to each entry point.
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    hipError_t alloc(size_t n) {
        n = n ? n : 16;
        if (n <= cap) return hipSuccess;
        if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
        const size_t want = n + n / 4;                       // head room: the next batch is rarely exactly this size
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) { e = hipMalloc(&p, n); if (e != hipSuccess) return e; cap = n; return e; }
        cap = want;
        return hipSuccess;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

// recorder for the next calls (hypo_gpu_profile_*): HIP events bound to the kernels' dispatches, no marker on a stream
struct ProfCall { int kind = 0; hypo::KernelEvents ke; };      // kind 1 = POA, 2 = scan
struct Prof { std::vector<ProfCall> calls; int used = 0; };

// One context per device handed to hypo_gpu_init ("one context per device inside one process").  Each owns its
// stream, the POA side streams / events / plan read-back buffer, the grow-only arenas of the host-pointer entry points and
// the uploaded solid-kmer set.  A calling thread works on the context it selected with hypo_gpu_use_device (slot 0 by
// default); entry points lock that context only, so threads driving different devices never wait for each other.
struct Ctx {
    bool ready = false; int device = -1; int num_cus = 0; hipStream_t stream = nullptr;
    // Two batches of the host-pointer POA entry points can be in flight (hypo_gpu_poa_batch_begin / _end): each has its own
    // device buffers, workspace, stream and side streams, so the upload of one overlaps the kernels of the other.  Slot 0's
    // stream is `stream` (also used by the scan and by hypo_gpu_poa_batch_sharded).
    struct Slot {
        DevBuf arena[10]; hypo::PoaAux aux; hipStream_t stream = nullptr; bool busy = false; uint32_t n = 0; HypoPoaStats* stats_pinned = nullptr;
    } slots[2];
    DevBuf scan_arena[7];
    // resident window batch of hypo_gpu_arms_build (inputs, work arrays, the batch, consensus slots, POA workspace)
    // resident window batches built by the arm kernels: [0] SHORT windows (hypo_gpu_arms_build), [1] LONG windows (hypo_gpu_arms_build_long)
    struct ArmsSet { DevBuf arena[5]; HypoArmsSummary sum{}; bool ready = false; hypo::ArmsOut out{}; };
    ArmsSet arms[2];
    // the short reads of the contig batch in hand (hypo_gpu_reads_upload): the support kernels vote with them, hypo_gpu_arms_build
    // (reads == NULL) cuts them into arms
    struct DevReads {                                      // the arrays of a HypoArmsReads in device memory (reads_to_device)
        const uint32_t *rb = nullptr, *re = nullptr, *qae = nullptr, *cigar_off = nullptr, *cigar = nullptr, *file_rank = nullptr;
        const uint64_t* seq_off = nullptr; const uint8_t* reads2 = nullptr;
    };
    struct ResidentReads {
        DevBuf data, work; bool ready = false;
        uint32_t n = 0; uint64_t reads2_bytes = 0; uint32_t max_span = 0; uint64_t sum_span = 0;
        uint64_t total_len = 0;                            // the coordinate space the reads were checked against
        std::vector<uint32_t> ctg_min_rb, ctg_max_re;      // per contig index of read_contig: what its reads span (later calls check their tables against it)
        DevReads dev; const uint32_t* read_contig = nullptr;
    } rr;
    DevBuf solid_set; uint32_t solid_k = 0;            // hypo_gpu_solid_set_upload
    // hypo_gpu_kmer_count_begin .. _end: the count table (4^k counters of 1 or 2 bytes, exact size), the bytes of the call in hand,
    // and the histogram / popcount results
    struct KmerCount { void* table = nullptr; size_t table_bytes = 0; DevBuf in, misc; uint32_t k = 0, cov = 0, sat = 0; int wide = 0; };
    KmerCount kc;
    // hypo_gpu_edit_scripts: the pairs' bytes and offsets, per-pair results, the run pool, the long / wide lists with their counters,
    // and the move storage (and wide band values) of the pairs that do not fit the fast path's LDS.  Grow-only.
    // A call that answered HYPO_E_WORKSPACE keeps its results (`kept`: the per-pair results on the host, the runs in `pool`) until
    // the next call, which copies them out when it names the same batch.
    struct EditKept {
        bool valid = false; const char* a = nullptr; const char* b = nullptr; uint64_t a0 = 0, b0 = 0, n_runs = 0;
        std::vector<uint64_t> aoff, boff; std::vector<uint32_t> res;
    };
    // last_counts: what the last computing call did (hypo_gpu_edit_last_counts; numbers the host loop holds anyway)
    struct EditBufs { DevBuf a, b, a_off, b_off, res, pool, lists, ctr, moves, moves_off, vals, vals_off; EditKept kept; uint64_t last_counts[8] = {0, 0, 0, 0, 0, 0, 0, 0}; };
    EditBufs ed;
    // hypo_gpu_kset_begin .. _end: the hash table (exact size; replaced by a larger one when it grows), the number of keys in it, the
    // bytes / offsets / results of the call in hand, the two counters of the kernels; what the growths cost (HYPO_KSET_STATS).
    // hypo_gpu_kset_counts_enable: n_texts > 0, and `planes` (exact size, replaced with the table) holds the count bytes of the reads
    // and n_texts planes of copy bytes (kset_kernel.hpp); `marked`: a text has been marked, the set takes no more reads
    struct KSet {
        uint64_t* table = nullptr; uint64_t slots = 0, max_slots = 0, count = 0; uint32_t k = 0; DevBuf in, off, res, ctr;
        uint32_t growths = 0; double grow_s = 0; uint64_t peak_slots = 0;
        uint64_t max_bytes = 0; uint32_t n_texts = 0; uint32_t* planes = nullptr; bool marked = false;
        uint32_t min_count = 1;                            // hypo_gpu_kset_min_count: the queries answer against the keys counted at least this often
        uint64_t plane_bytes(uint64_t n_slots) const { return n_texts ? (1 + (uint64_t)n_texts) * hypo::ks_plane_words(n_slots) * 4 : 0; }
        double slot_bytes() const { return n_texts ? 9.0 + n_texts : 8.0; }      // what max_bytes caps, per slot
        hypo::KsetView view() const { return {table, slots, k, planes, min_count}; }   // what the queries' launchers read of the set
    };
    KSet ks;
    size_t mem_free_at_init = 0;                       // hipMemGetInfo when the context was created (default cap of the k-mer set)
    // hypo_gpu_solid_scan_keep: the marked positions (contig-local) and their k-mers stay on the device, one pair of exact-size
    // buffers per handle (the caller's contig number); hypo_gpu_support_kmers_kept votes against them
    struct KeptScan { void* kids = nullptr; uint32_t* spos = nullptr; uint64_t n = 0, n_bases = 0; uint32_t k = 0; bool used = false; };
    std::vector<KeptScan> kept;
    // released scans are parked, not freed: hipFree waits for the device and costs 0.1-0.3 ms a call — a contig batch of the 3 Gbp
    // run releases 50 scans (100 buffers) inside its vote call.  Freed together when 16 GB are parked, and at shutdown.
    std::vector<void*> kept_parked; size_t kept_parked_bytes = 0;
    int poa_flags = 0;                                 // hypo_gpu_set_option
    Bounce bounce;                                     // page-locked staging of large copies out of pageable memory (h2d below)
    std::vector<HypoWindow> sh_win; std::vector<uint64_t> sh_aoff, sh_off;   // rebased descriptors of this device's share (hypo_gpu_poa_batch_sharded)
    Prof prof;
    std::recursive_mutex mu;                           // recursive: the host-buffer variants call the device variants
};
constexpr int kMaxDevices = HYPO_MAX_DEVICES;
Ctx g_ctxs[kMaxDevices];
int g_nctx = 0;
std::mutex g_init_mu;                                  // init / shutdown only
thread_local int tl_slot = 0;
Ctx& cur() { return g_ctxs[(tl_slot >= 0 && tl_slot < kMaxDevices) ? tl_slot : 0]; }
#define g_ctx (cur())
#define g_prof (cur().prof)
#define HYPO_LOCKED() std::lock_guard<std::recursive_mutex> hypo_lock_(cur().mu)
// the device of the context is made current for the calling thread (hypo_gpu_init did that for its own thread only)
#define HYPO_ON_DEVICE() do { if (g_ctx.ready) HIP_TRY(hipSetDevice(g_ctx.device)); } while (0)
// How an entry point that works on the calling thread's context begins: its lock, its device, and that hypo_gpu_init made it.
#define HYPO_ENTRY() \
    HYPO_LOCKED(); \
    HYPO_ON_DEVICE(); \
    if (!g_ctx.ready) return fail(HYPO_E_NOTINIT, "hypo_gpu_init was not called")
// The votes also need the reads of hypo_gpu_reads_upload.
#define HYPO_VOTE_ENTRY() \
    HYPO_ENTRY(); \
    if (!g_ctx.rr.ready) return fail(HYPO_E_INVALID, "no resident reads: call hypo_gpu_reads_upload first")

// Host memory -> device memory on `st`.  On return the host range may be reused (as with hipMemcpyAsync out of pageable
// memory); when `src` is page-locked the copy is queued as it is and the caller's usual rule applies (leave it alone until the
// stream has been synchronised — every entry point that takes page-locked memory does that before it returns or says so).
hipError_t h2d(void* dst, const void* src, size_t bytes, hipStream_t st) {
    constexpr size_t kStagedFrom = (size_t)8 << 20;
    if (bytes < kStagedFrom) return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st);
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, src) == hipSuccess && at.type != hipMemoryTypeUnregistered) return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st);
    (void)hipGetLastError();                           // (an ordinary pointer is "invalid" to that query)
    Ctx& c = cur();
    hipError_t e = c.bounce.ensure();
    if (e != hipSuccess) { (void)hipGetLastError(); return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st); }
    std::lock_guard<std::mutex> lk(g_copy_mu);
    Bounce& b = c.bounce;
    for (size_t at0 = 0; at0 < bytes; at0 += Bounce::kChunk) {
        const size_t n = bytes - at0 < Bounce::kChunk ? bytes - at0 : Bounce::kChunk;
        const int i = b.turn; b.turn ^= 1;
        if (b.used[i] && (e = hipEventSynchronize(b.ev[i])) != hipSuccess) return e;      // the copy that last read this buffer has left it
        g_copy_pool.copy((char*)b.buf[i], (const char*)src + at0, n);
        if ((e = hipMemcpyAsync((char*)dst + at0, b.buf[i], n, hipMemcpyHostToDevice, st)) != hipSuccess) return e;
        if ((e = hipEventRecord(b.ev[i], st)) != hipSuccess) return e;
        b.used[i] = true;
    }
    return hipSuccess;
}

// Device memory -> host memory behind what is queued on `st`; the data is in `dst` on return.  The way back of h2d: the DMA engine
// fills one bounce buffer while the copy threads empty the other into the caller's ordinary memory (160 MB of vote counters per
// 50 Mbp batch of the 3 Gbp run come back this way).  Page-locked `dst`: copied into directly (queued; the caller synchronises).
hipError_t d2h(void* dst, const void* src, size_t bytes, hipStream_t st) {
    constexpr size_t kStagedFrom = (size_t)8 << 20;
    if (bytes < kStagedFrom) return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st);
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, dst) == hipSuccess && at.type != hipMemoryTypeUnregistered) return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st);
    (void)hipGetLastError();
    Ctx& c = cur();
    hipError_t e = c.bounce.ensure();
    if (e != hipSuccess) { (void)hipGetLastError(); return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st); }
    std::lock_guard<std::mutex> lk(g_copy_mu);
    Bounce& b = c.bounce;
    size_t prev_at = 0, prev_n = 0; int prev_i = -1;
    for (size_t at0 = 0; at0 < bytes; at0 += Bounce::kChunk) {
        const size_t n = bytes - at0 < Bounce::kChunk ? bytes - at0 : Bounce::kChunk;
        const int i = b.turn; b.turn ^= 1;
        if (b.used[i] && (e = hipEventSynchronize(b.ev[i])) != hipSuccess) return e;      // (an upload that last read this buffer)
        if ((e = hipMemcpyAsync(b.buf[i], (const char*)src + at0, n, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
        if ((e = hipEventRecord(b.ev[i], st)) != hipSuccess) return e;
        b.used[i] = true;
        if (prev_i >= 0) {                                                                 // empty the other buffer while this one fills
            if ((e = hipEventSynchronize(b.ev[prev_i])) != hipSuccess) return e;
            g_copy_pool.copy((char*)dst + prev_at, (const char*)b.buf[prev_i], prev_n);
        }
        prev_i = i; prev_at = at0; prev_n = n;
    }
    if (prev_i >= 0) {
        if ((e = hipEventSynchronize(b.ev[prev_i])) != hipSuccess) return e;
        g_copy_pool.copy((char*)dst + prev_at, (const char*)b.buf[prev_i], prev_n);
    }
    return hipSuccess;
}

ProfCall* prof_next(int kind) {
    if (g_prof.used >= (int)g_prof.calls.size()) return nullptr;
    ProfCall* c = &g_prof.calls[g_prof.used++];
    c->kind = kind; c->ke.n = 0; c->ke.bound = 0;
    return c;
}

struct Rccl {
    void* h = nullptr; bool tried = false; bool ok = false;
    int (*CommInitAll)(void**, int, const int*) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    int (*Broadcast)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    void* comms[kMaxDevices] = {};
    int n_comms = 0; int devs[kMaxDevices] = {};
    bool load() {
        if (tried) return ok;
        tried = true;
        for (const char* name : {"librccl.so.1", "librccl.so"}) { h = dlopen(name, RTLD_NOW | RTLD_GLOBAL); if (h) break; }
        if (!h) return false;
        CommInitAll = (int (*)(void**, int, const int*))dlsym(h, "ncclCommInitAll");
        CommDestroy = (int (*)(void*))dlsym(h, "ncclCommDestroy");
        GroupStart = (int (*)())dlsym(h, "ncclGroupStart");
        GroupEnd = (int (*)())dlsym(h, "ncclGroupEnd");
        Broadcast = (int (*)(const void*, void*, size_t, int, int, void*, hipStream_t))dlsym(h, "ncclBroadcast");
        GetErrorString = (const char* (*)(int))dlsym(h, "ncclGetErrorString");
        ok = CommInitAll && CommDestroy && GroupStart && GroupEnd && Broadcast && GetErrorString;
        return ok;
    }
    void release() { for (int i = 0; i < n_comms; ++i) if (comms[i] && CommDestroy) (void)CommDestroy(comms[i]); n_comms = 0; }
};
Rccl g_rccl;
std::mutex g_shard_mu;                               // one sharded call at a time (it uses every context)
constexpr int kNcclUint8 = 1;                         // ncclUint8 (rccl.h)


int check_k(uint32_t k) { return k < 2 || k > 31 ? fail(HYPO_E_INVALID, "k=%u out of range 2..31", k) : HYPO_OK; }

int check_scores(const HypoScoreParams* s) {
    if (!s) return fail(HYPO_E_INVALID, "scores == NULL");
    if (s->sr_gap > 0 || s->lr_gap > 0)
        return fail(HYPO_E_INVALID, "gap penalties must be non-positive (spoa alignment_engine.cpp:43-50)");
    return HYPO_OK;
}

hypo::PoaParams make_params(const HypoScoreParams* s, const HypoWindowBatch* in, HypoConsensusBatch* out) {
    hypo::PoaParams P;
    P.windows = in->windows; P.draft4 = in->draft4; P.arm_off = in->arm_off; P.arm_len = in->arm_len; P.arms2 = in->arms2;
    P.out_bases = out->bases; P.out_off = out->off; P.out_len = out->len; P.out_status = out->status;
    P.sr_m = s->sr_match; P.sr_n = s->sr_mismatch; P.sr_g = s->sr_gap;
    P.lr_m = s->lr_match; P.lr_n = s->lr_mismatch; P.lr_g = s->lr_gap;
    P.n_arms = in->n_arms; P.draft4_bytes = in->draft4_bytes; P.arms2_bytes = in->arms2_bytes;
    P.flags = g_ctx.poa_flags;
    return P;
}

struct Carver {                                       // lays arrays out in one device buffer, 256-byte aligned
    size_t at = 0;
    static size_t pad(size_t bytes) { return (bytes + 255) / 256 * 256; }
    size_t take(size_t bytes) { const size_t o = at; at += pad(bytes); return o; }
};

// A device buffer that a Carver laid out, on the stream that fills it: dev.u32(o) / .u64(o) / .u8(o) / .ull(o) / .at<T>(o) is the array at byte
// offset o with the element type named; dev.up(o, src, bytes) sends host memory there and dev.down(dst, o, bytes) brings it back
// (nothing for an empty array; h2d / d2h, so the stream is the one to synchronise).
struct DevAt {
    char* base; hipStream_t st;
    template <class T> T* at(size_t off) const { return (T*)(base + off); }
    uint32_t* u32(size_t off) const { return at<uint32_t>(off); }
    uint64_t* u64(size_t off) const { return at<uint64_t>(off); }
    uint8_t* u8(size_t off) const { return at<uint8_t>(off); }
    unsigned long long* ull(size_t off) const { return at<unsigned long long>(off); }   // (the type of the kernels' atomic sums)
    hipError_t up(size_t off, const void* src, size_t bytes) const { return bytes ? h2d(base + off, src, bytes, st) : hipSuccess; }
    hipError_t down(void* dst, size_t off, size_t bytes) const { return bytes ? d2h(dst, base + off, bytes, st) : hipSuccess; }
};

// ---- the alignment records of a HypoArmsReads: checked on the host, then on the device -------------------------------------------
// What is wrong with record a, in the order the checks are reported (0: nothing).  read_contig: NULL where the call has none.
// Inlined into both record loops: ten million records per contig batch go through it.
enum ReadFault { READ_OK = 0, READ_SPAN, READ_ORDER, READ_SEQ, READ_CIGAR, READ_CONTIG };
__attribute__((always_inline)) inline ReadFault read_fault(const HypoArmsReads& A, uint32_t a, uint64_t total_len, const uint32_t* read_contig) {
    if (A.re[a] <= A.rb[a] || A.re[a] > total_len) return READ_SPAN;
    if (a && A.rb[a - 1] > A.rb[a]) return READ_ORDER;
    if (A.seq_off[a] + ((uint64_t)A.qae[a] + 3) / 4 > A.reads2_bytes) return READ_SEQ;
    if (A.cigar_off[a] > A.cigar_off[a + 1]) return READ_CIGAR;
    if (read_contig && read_contig[a] >= 0x01000000u) return READ_CONTIG;
    return READ_OK;
}
int read_fail(ReadFault why, const HypoArmsReads& A, uint32_t a, uint64_t total_len, const uint32_t* read_contig) {
    switch (why) {
    case READ_SPAN: return fail(HYPO_E_INVALID, "alignment %u: span [%u, %u) outside the %llu bases", a, A.rb[a], A.re[a], (unsigned long long)total_len);
    case READ_ORDER: return fail(HYPO_E_INVALID, "alignments are not sorted by reference start (alignment %u)", a);
    case READ_SEQ: return fail(HYPO_E_INVALID, "alignment %u: read outside reads2", a);
    case READ_CIGAR: return fail(HYPO_E_INVALID, "alignment %u: cigar_off decreases", a);
    default: return fail(HYPO_E_INVALID, "alignment %u: contig index %u out of range", a, read_contig[a]);
    }
}

// The arrays of `A` behind what `c` holds already, in `buf` (sized here for all of it); `R` gets the device pointers.
int reads_to_device(Carver& c, DevBuf& buf, const HypoArmsReads& A, hipStream_t st, Ctx::DevReads& R) {
    const size_t na = A.n_alignments, n_cig = na ? A.cigar_off[na] : 0;
    const size_t o_rb = c.take(na * 4), o_re = c.take(na * 4), o_qae = c.take(na * 4), o_soff = c.take(na * 8), o_reads = c.take(A.reads2_bytes),
                 o_coff = c.take((na + 1) * 4), o_cig = c.take(n_cig * 4), o_rank = c.take(A.file_rank ? na * 4 : 0);
    HIP_TRY(buf.alloc(c.at));
    const DevAt d{(char*)buf.p, st};
    HIP_TRY(d.up(o_rb, A.rb, na * 4)); HIP_TRY(d.up(o_re, A.re, na * 4)); HIP_TRY(d.up(o_qae, A.qae, na * 4)); HIP_TRY(d.up(o_soff, A.seq_off, na * 8));
    HIP_TRY(d.up(o_reads, A.reads2, A.reads2_bytes)); if (na) HIP_TRY(d.up(o_coff, A.cigar_off, (na + 1) * 4)); HIP_TRY(d.up(o_cig, A.cigar, n_cig * 4));
    if (A.file_rank) HIP_TRY(d.up(o_rank, A.file_rank, na * 4));
    R.rb = d.u32(o_rb); R.re = d.u32(o_re); R.qae = d.u32(o_qae); R.seq_off = d.u64(o_soff); R.reads2 = d.u8(o_reads); R.cigar_off = d.u32(o_coff); R.cigar = d.u32(o_cig);
    R.file_rank = A.file_rank ? d.u32(o_rank) : nullptr;
    return HYPO_OK;
}

// What the three votes do alike once their tables are in `d`, whose tail from o_cov to `end` holds the two arrays of n counters:
// the counters zeroed, the entry's kernel through launch(cov, sup) (an error code: the entry names its own kernel in it), both arrays down to the host, the stream drained.
template <class Launch>
int vote_run(const DevAt& d, size_t o_cov, size_t o_sup, size_t end, uint64_t n, uint32_t* coverage, uint32_t* support, Launch launch) {
    HIP_TRY(hipMemsetAsync(d.u32(o_cov), 0, end - o_cov, d.st));
    if (const int rc = launch(d.u32(o_cov), d.u32(o_sup))) return rc;
    HIP_TRY(d2h(coverage, d.u32(o_cov), n * 4, d.st));
    HIP_TRY(d2h(support, d.u32(o_sup), n * 4, d.st));
    HIP_TRY(hipStreamSynchronize(d.st));
    return HYPO_OK;
}


// First-use costs of a HIP process — loading this library's code objects onto the device, the occupancy queries, the side
// streams and events of the POA call — come to ≈ 20–40 ms, several steady-state POA calls of the C2 batch, and used to land in
// whichever call came first.  hypo_gpu_init pays them once per context: a two-window batch, a 64-base scan and a four-element
// prefix sum on throw-away buffers.  HYPO_NO_WARMUP=1 leaves them to the first calls (profiles/diag/first_call.py measures
// the difference).
void warm_up(Ctx* c) {
    if (hipSetDevice(c->device) != hipSuccess) return;
    // On the HIP null stream, with side streams of its own that are destroyed again: a process gets four hardware queues by
    // default (GPU_MAX_HW_QUEUES), the POA call uses four streams (the caller's + three side streams), and a warm-up on a fifth
    // stream made two of them share a queue for the rest of the run — measured as a shifted balance of the three concurrent class
    // kernels, C2 step 3.70 -> 4.27 ms.  HYPO_WARMUP_STREAM=0 (diagnostic) runs it on the context's stream as before, 2 on a
    // stream that is created and destroyed here.
    const char* ws_env = getenv("HYPO_WARMUP_STREAM");
    const int ws_mode = ws_env ? atoi(ws_env) : 1;
    hipStream_t st = nullptr, own = nullptr;
    if (ws_mode == 0) st = c->stream;
    if (ws_mode == 2 && hipStreamCreateWithFlags(&own, hipStreamNonBlocking) == hipSuccess) st = own;
    const uint32_t nw = 2, na = 4;
    const size_t wsb = hypo::poa_workspace_bytes(nw, hypo::kMinGlobalGroups, 0), swb = hypo::scan_workspace_bytes(64);
    Carver cv;
    const size_t o_win = cv.take(nw * sizeof(HypoWindow)), o_dr = cv.take(64), o_aoff = cv.take(na * 8), o_alen = cv.take(na * 4), o_arms = cv.take(64),
                 o_bases = cv.take(256), o_off = cv.take((nw + 1) * 8), o_len = cv.take(nw * 4), o_st = cv.take(64), o_p4 = cv.take(64), o_bits = cv.take(64),
                 o_words = cv.take(64), o_kids = cv.take(64 * 8), o_rank = cv.take(64), o_n = cv.take(64), o_sws = cv.take(swb), o_scan = cv.take(64 * 8), o_ws = cv.take(wsb);
    char* d = nullptr;
    if (hipMalloc((void**)&d, cv.at) != hipSuccess) return;
    (void)hipMemsetAsync(d, 0, o_ws, st);                  // all-A drafts and arms, an empty 2-mer set
    HypoWindow hw[nw] = {};
    uint64_t aoff[na] = {0, 8, 16, 24}, off[nw + 1] = {0, 64, 128};
    uint32_t alen[na] = {24, 24, 24, 24};
    for (uint32_t w = 0; w < nw; ++w) { hw[w].type = HYPO_WIN_SHORT; hw[w].draft_len = 24; hw[w].draft_off = 16 * w; hw[w].first_arm = 2 * w; hw[w].n_internal = 2; }
    (void)hipMemcpyAsync(d + o_win, hw, sizeof(hw), hipMemcpyHostToDevice, st);
    (void)hipMemcpyAsync(d + o_aoff, aoff, sizeof(aoff), hipMemcpyHostToDevice, st);
    (void)hipMemcpyAsync(d + o_alen, alen, sizeof(alen), hipMemcpyHostToDevice, st);
    (void)hipMemcpyAsync(d + o_off, off, sizeof(off), hipMemcpyHostToDevice, st);
    (void)hypo::scan_run((const uint8_t*)(d + o_p4), 64, 2, (const uint64_t*)(d + o_bits), (uint64_t*)(d + o_words), (uint64_t*)(d + o_kids), 64, (uint64_t*)(d + o_rank),
                         (uint64_t*)(d + o_n), d + o_sws, swb, st, nullptr);
    hypo::PoaParams P;
    P.windows = (const HypoWindow*)(d + o_win); P.draft4 = (const uint8_t*)(d + o_dr); P.arm_off = (const uint64_t*)(d + o_aoff); P.arm_len = (const uint32_t*)(d + o_alen);
    P.arms2 = (const uint8_t*)(d + o_arms); P.out_bases = d + o_bases; P.out_off = (const uint64_t*)(d + o_off); P.out_len = (uint32_t*)(d + o_len); P.out_status = (uint8_t*)(d + o_st);
    P.sr_m = 5; P.sr_n = -4; P.sr_g = -8; P.lr_m = 3; P.lr_n = -5; P.lr_g = -4;
    P.n_arms = na; P.draft4_bytes = 64; P.arms2_bytes = 64; P.flags = 0;
    hypo::PoaAux tmp;
    (void)hypo::poa_run(P, nw, d + o_ws, wsb, c->num_cus, st, nullptr, &tmp);
    (void)hypo::scan32((const uint32_t*)(d + o_alen), na, (uint64_t*)(d + o_scan), (uint64_t*)(d + o_sws), (uint64_t*)(d + o_n), st);
    (void)hipStreamSynchronize(st);
    hypo::poa_release(&tmp);
    if (own) (void)hipStreamDestroy(own);
    (void)hipFree(d);
    (void)hipGetLastError();
}

}  // namespace

extern "C" {

int hypo_gpu_abi_version(void) { return HYPO_GPU_ABI_VERSION; }
const char* hypo_gpu_last_error(void) { return tl_err; }
int hypo_gpu_num_cus(void) { return g_ctx.ready ? g_ctx.num_cus : 0; }
int hypo_gpu_num_devices(void) { return g_nctx; }
#ifndef HYPO_BUILD_ID
#define HYPO_BUILD_ID "unknown"
#endif
const char* hypo_gpu_build_id(void) { return HYPO_BUILD_ID; }

static void release_ctx(Ctx& c) {
    if (c.ready) {
        (void)hipSetDevice(c.device);
        (void)hipDeviceSynchronize();
        for (auto& pc : c.prof.calls) for (auto& e : pc.ke.ev) if (e) (void)hipEventDestroy(e);
        c.prof.calls.clear(); c.prof.used = 0;
        for (auto& sl : c.slots) { hypo::poa_release(&sl.aux); for (auto& a : sl.arena) a.release(); sl.busy = false; if (sl.stats_pinned) (void)hipHostFree(sl.stats_pinned); sl.stats_pinned = nullptr; }
        if (c.slots[1].stream) (void)hipStreamDestroy(c.slots[1].stream);
        c.slots[0].stream = c.slots[1].stream = nullptr;
        for (auto& a : c.scan_arena) a.release();
        for (auto& as : c.arms) { for (auto& a : as.arena) a.release(); as.ready = false; }
        c.rr.data.release(); c.rr.work.release(); c.rr.ready = false;
        c.solid_set.release(); c.solid_k = 0;
        if (c.kc.table) (void)hipFree(c.kc.table);
        c.kc.in.release(); c.kc.misc.release(); c.kc = Ctx::KmerCount();
        for (DevBuf* d : {&c.ed.a, &c.ed.b, &c.ed.a_off, &c.ed.b_off, &c.ed.res, &c.ed.pool, &c.ed.lists, &c.ed.ctr, &c.ed.moves, &c.ed.moves_off, &c.ed.vals, &c.ed.vals_off}) d->release();
        c.ed.kept = Ctx::EditKept();
        memset(c.ed.last_counts, 0, sizeof c.ed.last_counts);
        if (c.ks.table) (void)hipFree(c.ks.table);
        if (c.ks.planes) (void)hipFree(c.ks.planes);
        for (DevBuf* d : {&c.ks.in, &c.ks.off, &c.ks.res, &c.ks.ctr}) d->release();
        c.ks = Ctx::KSet();
        c.bounce.release();
        for (auto& ks : c.kept) { if (ks.kids) (void)hipFree(ks.kids); if (ks.spos) (void)hipFree(ks.spos); }
        c.kept.clear();
        for (void* p : c.kept_parked) (void)hipFree(p);
        c.kept_parked.clear(); c.kept_parked_bytes = 0;
        if (c.stream) (void)hipStreamDestroy(c.stream);
    }
    c.ready = false; c.device = -1; c.num_cus = 0; c.stream = nullptr;
}

int hypo_gpu_init(const int* device_ids, int n_devices) {
    std::lock_guard<std::mutex> lk(g_init_mu);
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return fail(HYPO_E_NODEVICE, "no HIP device visible");
    const int zero = 0;
    if (!device_ids || n_devices <= 0) { device_ids = &zero; n_devices = 1; }       // (NULL, 0): device 0
    if (n_devices > kMaxDevices) return fail(HYPO_E_INVALID, "%d devices requested, at most %d", n_devices, kMaxDevices);
    for (int i = 0; i < n_devices; ++i) {
        if (device_ids[i] < 0 || device_ids[i] >= n) return fail(HYPO_E_INVALID, "device %d out of range (0..%d)", device_ids[i], n - 1);
        // HYPO_ALLOW_DUP_DEVICES=1 (tests on a one-GPU box): several contexts on one device exercise the sharded path
        for (int j = 0; j < i; ++j) if (device_ids[j] == device_ids[i] && !getenv("HYPO_ALLOW_DUP_DEVICES")) return fail(HYPO_E_INVALID, "device %d listed twice", device_ids[i]);
    }
    for (int i = 0; i < g_nctx; ++i) release_ctx(g_ctxs[i]);   // re-initialisation: streams and events belong to the previous devices
    g_nctx = 0;
    for (int i = 0; i < n_devices; ++i) {
        Ctx& c = g_ctxs[i];
        HIP_TRY(hipSetDevice(device_ids[i]));
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, device_ids[i]));
        if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
            return fail(HYPO_E_NODEVICE, "device %d is %s; this library is built for gfx950 only", device_ids[i], prop.gcnArchName);
        HIP_TRY(hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking));
        c.slots[0].stream = c.stream;                      // (slot 1's stream is created when a second batch is first put in flight)
        c.device = device_ids[i]; c.num_cus = prop.multiProcessorCount; c.ready = true;
        size_t mem_total = 0;
        if (hipMemGetInfo(&c.mem_free_at_init, &mem_total) != hipSuccess) { (void)hipGetLastError(); c.mem_free_at_init = 0; }
        g_nctx = i + 1;
    }
    if (!getenv("HYPO_NO_WARMUP")) for (int i = 0; i < g_nctx; ++i) warm_up(&g_ctxs[i]);
    HIP_TRY(hipSetDevice(g_ctxs[0].device));
    tl_slot = 0;
    return HYPO_OK;
}

// hypo_gpu_set_option("edit_chunk_mb"): move storage per launch of the long / wide paths of hypo_gpu_edit_scripts (more when one pair needs it)
static std::atomic<uint64_t> g_edit_chunk_bytes{(uint64_t)256 << 20};

int hypo_gpu_set_option(const char* name, int value) {
    if (!name) return fail(HYPO_E_INVALID, "NULL option name");
    if (!strcmp(name, "native_klov")) {                  // all contexts: the mode belongs to the run, not to a device
        for (int i = 0; i < kMaxDevices; ++i) g_ctxs[i].poa_flags = (g_ctxs[i].poa_flags & ~hypo::POA_NATIVE_KLOV) | (value ? hypo::POA_NATIVE_KLOV : 0);
        return HYPO_OK;
    }
    if (!strcmp(name, "poa_min_class")) {                // 0 .. 3: SHORT windows start in at least this size class (parity sweeps: every class's code on small windows)
        if (value < 0 || value > 3) return fail(HYPO_E_INVALID, "poa_min_class %d out of range 0..3", value);
        for (int i = 0; i < kMaxDevices; ++i) g_ctxs[i].poa_flags = (g_ctxs[i].poa_flags & ~(3 << hypo::POA_MIN_CLASS_SHIFT)) | (value << hypo::POA_MIN_CLASS_SHIFT);
        return HYPO_OK;
    }
    if (!strcmp(name, "giant_arena_mb")) {               // HBM of size class 6 per POA context created from now on (poa_giant.hpp); 0 = none
        if (value < 0 || value > (1 << 20)) return fail(HYPO_E_INVALID, "giant_arena_mb %d out of range", value);
        hypo::poa_set_giant_arena_mb(value);
        return HYPO_OK;
    }
    if (!strcmp(name, "edit_chunk_mb")) {                // move storage per launch of the long / wide edit paths; results do not depend on it
        if (value < 1 || value > 4096) return fail(HYPO_E_INVALID, "edit_chunk_mb %d out of range 1..4096", value);
        g_edit_chunk_bytes = (uint64_t)value << 20;
        return HYPO_OK;
    }
    return fail(HYPO_E_INVALID, "unknown option %s", name);
}

int hypo_gpu_use_device(int slot) {
    if (slot < 0 || slot >= g_nctx) return fail(HYPO_E_INVALID, "context %d out of range (hypo_gpu_init created %d)", slot, g_nctx);
    tl_slot = slot;
    HIP_TRY(hipSetDevice(g_ctxs[slot].device));
    return HYPO_OK;
}

int hypo_gpu_shutdown(void) {
    std::lock_guard<std::mutex> lk(g_init_mu);
    g_rccl.release();
    for (int i = 0; i < g_nctx; ++i) release_ctx(g_ctxs[i]);
    g_nctx = 0;
    return HYPO_OK;
}

// ---- profiling ---------------------------------------------------------------------------------------
int hypo_gpu_profile_begin(int max_calls) {
    HYPO_LOCKED();
    if (!g_ctx.ready) return fail(HYPO_E_NOTINIT, "hypo_gpu_init was not called");
    if (max_calls < 0 || max_calls > 256) return fail(HYPO_E_INVALID, "max_calls out of range 0..256");
    for (auto& c : g_prof.calls) for (auto& e : c.ke.ev) if (e) (void)hipEventDestroy(e);
    g_prof.calls.assign((size_t)max_calls, ProfCall());
    g_prof.used = 0;
    // (the events only carry times: no system-scope release at the end of the kernel one is bound to)
    for (auto& c : g_prof.calls) for (auto& e : c.ke.ev) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableSystemFence));
    return HYPO_OK;
}
int hypo_gpu_profile_calls(void) { return g_prof.used; }
int hypo_gpu_profile_read(int call, float* ms, int n) {
    HYPO_LOCKED();
    if (call < 0 || call >= g_prof.used || !ms) return fail(HYPO_E_INVALID, "no such profiled call");
    ProfCall& c = g_prof.calls[(size_t)call];
    if (c.ke.n < 2) return 0;
    HIP_TRY(hipEventSynchronize(c.ke.ev[c.kind == 1 ? c.ke.n - 1 : 1]));
    int out = 0;
    float t = 0.f;
    if (c.kind == 1) {          // POA: [plan, class 0..5, whole call]; the kernels of the pairs may sit on different streams
        const int pairs = (c.ke.n - 1) / 2;
        for (int i = 0; i < pairs && out < n; ++i) {
            t = 0.f;                                           // (a class without a timed launch in this call: KernelEvents::bound)
            if (i == 0 || (c.ke.bound >> (2 * i)) & 1u) {
                HIP_TRY(hipEventSynchronize(c.ke.ev[2 * i + 1]));
                HIP_TRY(hipEventElapsedTime(&t, c.ke.ev[2 * i], c.ke.ev[2 * i + 1]));
            }
            ms[out++] = t;
        }
        if (out < n) { HIP_TRY(hipEventElapsedTime(&t, c.ke.ev[0], c.ke.ev[c.ke.n - 1])); ms[out++] = t; }
        return out;
    }
    // scan: [the scan kernel, 0, 0] (the two zeros keep the record's length: they timed nothing but event records since round 5)
    HIP_TRY(hipEventElapsedTime(&t, c.ke.ev[0], c.ke.ev[1]));
    for (int i = 0; i + 1 < c.ke.n && out < n; ++i) ms[out++] = i == 0 ? t : 0.f;
    return out;
}

// ---- POA -------------------------------------------------------------------------------------------
size_t hypo_gpu_poa_workspace_bytes(uint32_t n_windows, uint32_t n_arms) {
    return hypo::poa_workspace_bytes(n_windows, 0, n_arms);       // room for arm offsets computed on the device (arm_off == NULL)
}

int hypo_gpu_poa_batch_device(const HypoScoreParams* scores, const HypoWindowBatch* in, HypoConsensusBatch* out,
                              void* workspace, size_t workspace_bytes, void* hip_stream) {
    HYPO_ENTRY();
    int rc = check_scores(scores);
    if (rc) return rc;
    if (!in || !out) return fail(HYPO_E_INVALID, "NULL batch");
    if (in->n_windows == 0) return HYPO_OK;
    if (!in->windows || !in->draft4 || !out->bases || !out->off || !out->len || !out->status ||
        (in->n_arms && (!in->arm_len || !in->arms2)))
        return fail(HYPO_E_INVALID, "NULL buffer in batch");
    if (!workspace || workspace_bytes < hypo::poa_workspace_bytes(in->n_windows, hypo::kMinGlobalGroups, in->arm_off ? 0 : in->n_arms))
        return fail(HYPO_E_WORKSPACE, "workspace %zu < minimum %zu (hypo_gpu_poa_workspace_bytes recommends %zu)", workspace_bytes,
                    hypo::poa_workspace_bytes(in->n_windows, hypo::kMinGlobalGroups, in->arm_off ? 0 : in->n_arms), hypo::poa_workspace_bytes(in->n_windows, 0, in->n_arms));
    hypo::PoaParams P = make_params(scores, in, out);
    hipStream_t st = (hipStream_t)hip_stream;                  // NULL is the HIP null stream itself (what torch calls its default stream)
    ProfCall* pc = prof_next(1);
    HIP_TRY(hypo::poa_run(P, in->n_windows, workspace, workspace_bytes, g_ctx.num_cus, st, pc ? &pc->ke : nullptr, &g_ctx.slots[0].aux));
    return HYPO_OK;
}

// device-side stats of the last device call live at workspace + 128
int hypo_gpu_poa_read_stats(const void* workspace, void* hip_stream, HypoPoaStats* out) {
    if (!g_ctx.ready) return fail(HYPO_E_NOTINIT, "hypo_gpu_init was not called");
    hipStream_t st = (hipStream_t)hip_stream;                  // NULL is the HIP null stream itself (what torch calls its default stream)
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipMemcpy(out, (const char*)workspace + 128, sizeof(HypoPoaStats), hipMemcpyDeviceToHost));
    return HYPO_OK;
}

int hypo_gpu_poa_last_stats(HypoPoaStats* out) {
    if (!out) return fail(HYPO_E_INVALID, "NULL");
    *out = tl_stats;
    return HYPO_OK;
}

int hypo_gpu_poa_slot_layout(const HypoWindowBatch* in, uint64_t* off) {
    if (!in || !off) return fail(HYPO_E_INVALID, "NULL");
    uint64_t acc = 0;
    for (uint32_t w = 0; w < in->n_windows; ++w) {
        const HypoWindow& W = in->windows[w];
        uint64_t longest = W.draft_len;
        const uint64_t narm = (uint64_t)W.n_internal + W.n_prefix + W.n_suffix;
        if (W.first_arm + narm > in->n_arms) return fail(HYPO_E_INVALID, "window %u: arms [%u, %llu) outside the batch's %u arms", w, W.first_arm, (unsigned long long)(W.first_arm + narm), in->n_arms);
        for (uint64_t a = 0; a < narm; ++a) if (in->arm_len[W.first_arm + a] > longest) longest = in->arm_len[W.first_arm + a];
        off[w] = acc;
        acc += (longest + longest / 2 + 24 + 7) / 8 * 8;
    }
    off[in->n_windows] = acc;
    return HYPO_OK;
}

// Queues one batch: upload, kernels, download of the results into the caller's buffers, all on the slot's stream; returns
// without waiting.  `in` and `out` buffers must stay untouched until hypo_gpu_poa_batch_end(ticket).
int hypo_gpu_poa_batch_begin(const HypoScoreParams* scores, const HypoWindowBatch* in, HypoConsensusBatch* out, int* ticket) {
    HYPO_ENTRY();
    int rc = check_scores(scores);
    if (rc) return rc;
    if (!in || !out || !ticket) return fail(HYPO_E_INVALID, "NULL batch");
    const uint32_t n = in->n_windows, na = in->n_arms;
    if (n && (!in->windows || !in->draft4 || !out->bases || !out->off || !out->len || !out->status || (na && (!in->arm_len || !in->arms2))))
        return fail(HYPO_E_INVALID, "NULL buffer in batch");
    int si = -1;
    for (int i = 0; i < 2; ++i) if (!g_ctx.slots[i].busy) { si = i; break; }
    if (si < 0) return fail(HYPO_E_INVALID, "two batches are already in flight on this context: call hypo_gpu_poa_batch_end first");
    Ctx::Slot& S = g_ctx.slots[si];
    S.n = n;
    *ticket = si;
    S.busy = true;
    if (n == 0) return HYPO_OK;
    const uint64_t out_bytes = out->off[n];
    DevBuf &dW = S.arena[0], &dD = S.arena[1], &dAO = S.arena[2], &dAL = S.arena[3], &dA = S.arena[4],
           &dB = S.arena[5], &dO = S.arena[6], &dL = S.arena[7], &dS = S.arena[8], &dWS = S.arena[9];
    // the host sees the window types: scratch for as many resident LONG groups as there are LONG windows (+ escalations)
    uint32_t n_long = 0;
    for (uint32_t w = 0; w < n; ++w) n_long += in->windows[w].type != HYPO_WIN_SHORT;
    const size_t wsb = hypo::poa_workspace_bytes(n, (int)(n_long + 64 < 2048u ? n_long + 64 : 2048u), in->arm_off ? 0 : na);
    auto undo = [&](int code) { S.busy = false; return code; };
#define HIP_TRY_S(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return undo(fail(HYPO_E_HIP, "%s: %s", #x, hipGetErrorString(e_))); } while (0)
    HIP_TRY_S(dW.alloc((size_t)n * sizeof(HypoWindow))); HIP_TRY_S(dD.alloc(in->draft4_bytes));
    if (in->arm_off) HIP_TRY_S(dAO.alloc((size_t)na * 8));
    HIP_TRY_S(dAL.alloc((size_t)na * 4)); HIP_TRY_S(dA.alloc(in->arms2_bytes));
    HIP_TRY_S(dB.alloc(out_bytes)); HIP_TRY_S(dO.alloc((size_t)(n + 1) * 8)); HIP_TRY_S(dL.alloc((size_t)n * 4));
    HIP_TRY_S(dS.alloc(n)); HIP_TRY_S(dWS.alloc(wsb));
    if (!S.stream) HIP_TRY_S(hipStreamCreateWithFlags(&S.stream, hipStreamNonBlocking));
    if (!S.stats_pinned) HIP_TRY_S(hipHostMalloc((void**)&S.stats_pinned, sizeof(HypoPoaStats), hipHostMallocDefault));
    hipStream_t st = S.stream;
    HIP_TRY_S(h2d(dW.p, in->windows, (size_t)n * sizeof(HypoWindow), st));
    HIP_TRY_S(h2d(dD.p, in->draft4, in->draft4_bytes, st));
    if (na) {
        if (in->arm_off) HIP_TRY_S(hipMemcpyAsync(dAO.p, in->arm_off, (size_t)na * 8, hipMemcpyHostToDevice, st));
        HIP_TRY_S(hipMemcpyAsync(dAL.p, in->arm_len, (size_t)na * 4, hipMemcpyHostToDevice, st));
        HIP_TRY_S(h2d(dA.p, in->arms2, in->arms2_bytes, st));
    }
    HIP_TRY_S(hipMemcpyAsync(dO.p, out->off, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, st));
    HIP_TRY_S(hipMemsetAsync(dB.p, 0, out_bytes ? out_bytes : 16, st));   // slack bytes of a slot come back as 0
    HypoWindowBatch din = *in;
    din.windows = (const HypoWindow*)dW.p; din.draft4 = (const uint8_t*)dD.p; din.arm_off = in->arm_off ? (const uint64_t*)dAO.p : nullptr;
    din.arm_len = (const uint32_t*)dAL.p; din.arms2 = (const uint8_t*)dA.p;
    HypoConsensusBatch dout;
    dout.bases = (char*)dB.p; dout.off = (const uint64_t*)dO.p; dout.len = (uint32_t*)dL.p; dout.status = (uint8_t*)dS.p;
    hypo::PoaParams P = make_params(scores, &din, &dout);
    // both slots share the side streams, events and plan history of slot 0: the runtime maps streams onto a handful of hardware
    // queues, and every extra stream ends up sharing one with a size-class kernel (measured: classes 0 and 1 serialised)
    HIP_TRY_S(hypo::poa_run(P, n, dWS.p, wsb, g_ctx.num_cus, st, nullptr, &g_ctx.slots[0].aux));
    HIP_TRY_S(hipMemcpyAsync(out->bases, dB.p, out_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY_S(hipMemcpyAsync(out->len, dL.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY_S(hipMemcpyAsync(out->status, dS.p, n, hipMemcpyDeviceToHost, st));
    HIP_TRY_S(hipMemcpyAsync(S.stats_pinned, (char*)dWS.p + 128, sizeof(HypoPoaStats), hipMemcpyDeviceToHost, st));   // (page-locked: a copy into pageable memory would wait for the whole batch here)
#undef HIP_TRY_S
    return HYPO_OK;
}

int hypo_gpu_poa_batch_end(int ticket) {
    if (!g_ctx.ready) return fail(HYPO_E_NOTINIT, "hypo_gpu_init was not called");
    if (ticket < 0 || ticket > 1 || !g_ctx.slots[ticket].busy) return fail(HYPO_E_INVALID, "no batch in flight under ticket %d", ticket);
    Ctx::Slot& S = g_ctx.slots[ticket];
    HYPO_ON_DEVICE();
    const hipError_t e = S.n ? hipStreamSynchronize(S.stream) : hipSuccess;      // (no context lock while waiting: the other slot stays usable)
    HYPO_LOCKED();
    S.busy = false;
    if (e != hipSuccess) return fail(HYPO_E_HIP, "hipStreamSynchronize: %s", hipGetErrorString(e));
    if (S.n && S.stats_pinned) tl_stats = *S.stats_pinned; else memset(&tl_stats, 0, sizeof(tl_stats));
    tl_stats.n_windows = S.n;
    return HYPO_OK;
}

int hypo_gpu_poa_batch(const HypoScoreParams* scores, const HypoWindowBatch* in, HypoConsensusBatch* out) {
    memset(&tl_stats, 0, sizeof(tl_stats));
    int ticket = -1;
    const int rc = hypo_gpu_poa_batch_begin(scores, in, out, &ticket);
    if (rc) return rc;
    return hypo_gpu_poa_batch_end(ticket);
}

// ---- POA over all contexts ----------------------------------------------------------------------------
// Windows are independent (src/Hypo.cpp:238-247 is a parallel loop over them): the batch is cut into one contiguous,
// cost-balanced range per device, every device polishes its range, and the consensus bytes, lengths and status bytes are
// exchanged with ONE grouped RCCL all-gatherv over xGMI (ncclBroadcast per owner inside a group: the ranges differ in
// size) so that every device, device 0 in particular, holds the whole result before it goes back to the host for contig
// re-assembly (src/Contig.cpp:345-366).  RCCL is loaded on first use (a single-device run never touches it).
namespace {
struct Share { uint32_t w0 = 0, w1 = 0; uint64_t a0 = 0, a1 = 0, d0 = 0, d1 = 0, b0 = 0, b1 = 0; int rc = HYPO_OK; char err[256] = ""; HypoPoaStats st; };

// cost of a window as the plan sees it (rows x sequences), LONG windows twice
inline uint64_t window_cost(const HypoWindowBatch* in, uint32_t w) {
    const HypoWindow& W = in->windows[w];
    const uint64_t narm = (uint64_t)W.n_internal + W.n_prefix + W.n_suffix;
    uint64_t s = 0;
    if ((uint64_t)W.first_arm + narm <= in->n_arms) for (uint64_t a = 0; a < narm; ++a) s += in->arm_len[W.first_arm + a] + 1;
    return ((uint64_t)W.draft_len + 2) * (s + 1) * (W.type != HYPO_WIN_SHORT ? 2 : 1) + 64;
}
}  // namespace

int hypo_gpu_poa_batch_sharded(const HypoScoreParams* scores, const HypoWindowBatch* in, HypoConsensusBatch* out) {
    const int nd = g_nctx;
    if (nd <= 0) return fail(HYPO_E_NOTINIT, "hypo_gpu_init was not called");
    if (nd == 1 && !getenv("HYPO_MULTI_GATHER")) { const int keep = tl_slot; tl_slot = 0; const int rc = hypo_gpu_poa_batch(scores, in, out); tl_slot = keep; return rc; }
    std::lock_guard<std::mutex> shard_lock(g_shard_mu);
    int rc = check_scores(scores);
    if (rc) return rc;
    if (!in || !out) return fail(HYPO_E_INVALID, "NULL batch");
    memset(&tl_stats, 0, sizeof(tl_stats));
    const uint32_t n = in->n_windows;
    if (n == 0) return HYPO_OK;
    if (!in->windows || !in->draft4 || !out->bases || !out->off || !out->len || !out->status ||
        (in->n_arms && (!in->arm_off || !in->arm_len || !in->arms2)))
        return fail(HYPO_E_INVALID, "NULL buffer in batch");
    // ---- 1. contiguous cost-balanced ranges: per-chunk costs on nd threads, then a short prefix walk ----
    std::vector<uint64_t> cost(n);
    {
        std::vector<std::thread> th;
        for (int t = 0; t < nd; ++t) th.emplace_back([&, t]() {
            const uint32_t lo = (uint32_t)((uint64_t)n * t / nd), hi = (uint32_t)((uint64_t)n * (t + 1) / nd);
            for (uint32_t w = lo; w < hi; ++w) cost[w] = window_cost(in, w);
        });
        for (auto& t : th) t.join();
    }
    uint64_t total = 0;
    for (uint32_t w = 0; w < n; ++w) total += cost[w];
    std::vector<Share> sh((size_t)nd);
    {
        uint64_t acc = 0; uint32_t w = 0;
        for (int d = 0; d < nd; ++d) {
            sh[d].w0 = w;
            const uint64_t target = total / nd * (uint64_t)(d + 1) + (d + 1 == nd ? total % nd : 0);
            while (w < n && (d + 1 == nd || acc + cost[w] / 2 < target)) acc += cost[w++];
            sh[d].w1 = w;
        }
    }
    // ---- 2. every device: rebase its descriptors, upload its slices, run ----
    const bool want_rccl = nd > 1 ? !(getenv("HYPO_MULTI_GATHER") && !strcmp(getenv("HYPO_MULTI_GATHER"), "direct"))
                                  : (getenv("HYPO_MULTI_GATHER") && !strcmp(getenv("HYPO_MULTI_GATHER"), "rccl"));
    bool use_rccl = want_rccl && g_rccl.load();
    if (use_rccl) {                                    // communicators for the current device list (created once)
        bool same = g_rccl.n_comms == nd;
        for (int d = 0; same && d < nd; ++d) same = g_rccl.devs[d] == g_ctxs[d].device;
        if (!same) {
            g_rccl.release();
            int devs[kMaxDevices];
            for (int d = 0; d < nd; ++d) devs[d] = g_rccl.devs[d] = g_ctxs[d].device;
            const int r = g_rccl.CommInitAll(g_rccl.comms, nd, devs);
            if (r != 0) { fprintf(stderr, "[hypo_gpu] RCCL unavailable for this device list (%s): results go back per device\n", g_rccl.GetErrorString(r)); use_rccl = false; }
            else g_rccl.n_comms = nd;
        }
    }
    const uint64_t out_bytes = out->off[n];
    auto device_part = [&](int d) {
        Share& S = sh[d];
        Ctx& c = g_ctxs[d];
        std::lock_guard<std::recursive_mutex> lk(c.mu);
        auto bad = [&](int code, const char* what, hipError_t e) { S.rc = code; snprintf(S.err, sizeof(S.err), "device %d: %s: %s", c.device, what, hipGetErrorString(e)); };
        hipError_t e = hipSetDevice(c.device);
        if (e != hipSuccess) return bad(HYPO_E_HIP, "hipSetDevice", e);
        const uint32_t nw = S.w1 - S.w0;
        // result buffers of the WHOLE batch on every device (the gather fills the other devices' ranges)
        DevBuf* const ar = c.slots[0].arena;
        DevBuf &dW = ar[0], &dD = ar[1], &dAO = ar[2], &dAL = ar[3], &dA = ar[4], &dB = ar[5], &dO = ar[6], &dL = ar[7], &dS = ar[8], &dWS = ar[9];
        if ((e = dB.alloc(out_bytes)) != hipSuccess || (e = dL.alloc((size_t)n * 4)) != hipSuccess || (e = dS.alloc(n)) != hipSuccess)
            return bad(HYPO_E_HIP, "hipMalloc", e);
        memset(&S.st, 0, sizeof(S.st));
        if (nw == 0) return;
        // ranges of the shared buffers this share touches
        uint64_t a0 = ~0ull, a1 = 0, d0 = ~0ull, d1 = 0;
        for (uint32_t w = S.w0; w < S.w1; ++w) {
            const HypoWindow& W = in->windows[w];
            const uint64_t narm = (uint64_t)W.n_internal + W.n_prefix + W.n_suffix;
            if (narm && (uint64_t)W.first_arm + narm <= in->n_arms) { a0 = W.first_arm < a0 ? W.first_arm : a0; a1 = W.first_arm + narm > a1 ? W.first_arm + narm : a1; }
            if (W.draft_off <= in->draft4_bytes) {
                const uint64_t de = W.draft_off + ((uint64_t)W.draft_len + 1) / 2;
                d0 = W.draft_off < d0 ? W.draft_off : d0; d1 = (de < in->draft4_bytes ? de : in->draft4_bytes) > d1 ? (de < in->draft4_bytes ? de : in->draft4_bytes) : d1;
            }
        }
        if (a0 == ~0ull) { a0 = 0; a1 = 0; }
        if (d0 == ~0ull) { d0 = 0; d1 = 0; }
        uint64_t b0 = ~0ull, b1 = 0;
        for (uint64_t a = a0; a < a1; ++a) {
            const uint64_t o = in->arm_off[a], e2 = o + ((uint64_t)in->arm_len[a] + 3) / 4;
            if (o > in->arms2_bytes) continue;                 // left as it is: the device answers the window with HYPO_ST_INVALID
            b0 = o < b0 ? o : b0; b1 = (e2 < in->arms2_bytes ? e2 : in->arms2_bytes) > b1 ? (e2 < in->arms2_bytes ? e2 : in->arms2_bytes) : b1;
        }
        if (b0 == ~0ull) { b0 = 0; b1 = 0; }
        S.a0 = a0; S.a1 = a1; S.d0 = d0; S.d1 = d1; S.b0 = b0; S.b1 = b1;
        c.sh_win.assign(in->windows + S.w0, in->windows + S.w1);
        for (auto& W : c.sh_win) {
            // a window without arms does not take part in [a0, a1): its first_arm is rebased to 0 when it was valid in the whole
            // batch (the single-device call answers it with an empty consensus or its draft) and stays out of range otherwise
            if ((uint64_t)W.n_internal + W.n_prefix + W.n_suffix == 0) W.first_arm = (uint64_t)W.first_arm <= in->n_arms ? 0u : 0xffffffffu;
            else W.first_arm -= (uint32_t)(W.first_arm >= a0 ? a0 : 0);
            W.draft_off -= (W.draft_off >= d0 ? d0 : 0);
        }
        c.sh_aoff.resize((size_t)(a1 - a0));
        for (uint64_t a = a0; a < a1; ++a) c.sh_aoff[(size_t)(a - a0)] = in->arm_off[a] >= b0 ? in->arm_off[a] - b0 : in->arm_off[a];
        c.sh_off.resize((size_t)nw + 1);
        for (uint32_t i = 0; i <= nw; ++i) c.sh_off[i] = out->off[S.w0 + i];      // GLOBAL slot offsets: results land where the gather expects them
        uint32_t n_long = 0;
        for (const auto& W : c.sh_win) n_long += W.type != HYPO_WIN_SHORT;
        const size_t wsb = hypo::poa_workspace_bytes(nw, (int)(n_long + 64 < 2048u ? n_long + 64 : 2048u));
        if ((e = dW.alloc((size_t)nw * sizeof(HypoWindow))) != hipSuccess || (e = dD.alloc(d1 - d0)) != hipSuccess ||
            (e = dAO.alloc((a1 - a0) * 8)) != hipSuccess || (e = dAL.alloc((a1 - a0) * 4)) != hipSuccess ||
            (e = dA.alloc(b1 - b0)) != hipSuccess || (e = dO.alloc(((size_t)nw + 1) * 8)) != hipSuccess || (e = dWS.alloc(wsb)) != hipSuccess)
            return bad(HYPO_E_HIP, "hipMalloc", e);
        hipStream_t st = c.stream;
        (void)hipMemcpyAsync(dW.p, c.sh_win.data(), (size_t)nw * sizeof(HypoWindow), hipMemcpyHostToDevice, st);
        if (d1 > d0) (void)hipMemcpyAsync(dD.p, in->draft4 + d0, d1 - d0, hipMemcpyHostToDevice, st);
        if (a1 > a0) {
            (void)hipMemcpyAsync(dAO.p, c.sh_aoff.data(), (a1 - a0) * 8, hipMemcpyHostToDevice, st);
            (void)hipMemcpyAsync(dAL.p, in->arm_len + a0, (a1 - a0) * 4, hipMemcpyHostToDevice, st);
            if (b1 > b0) (void)hipMemcpyAsync(dA.p, in->arms2 + b0, b1 - b0, hipMemcpyHostToDevice, st);
        }
        (void)hipMemcpyAsync(dO.p, c.sh_off.data(), ((size_t)nw + 1) * 8, hipMemcpyHostToDevice, st);
        (void)hipMemsetAsync((char*)dB.p + out->off[S.w0], 0, out->off[S.w1] - out->off[S.w0] ? out->off[S.w1] - out->off[S.w0] : 1, st);
        if ((e = hipGetLastError()) != hipSuccess) return bad(HYPO_E_HIP, "upload", e);
        hypo::PoaParams P;
        P.windows = (const HypoWindow*)dW.p; P.draft4 = (const uint8_t*)dD.p; P.arm_off = (const uint64_t*)dAO.p;
        P.arm_len = (const uint32_t*)dAL.p; P.arms2 = (const uint8_t*)dA.p;
        P.out_bases = (char*)dB.p; P.out_off = (const uint64_t*)dO.p;
        P.out_len = (uint32_t*)dL.p + S.w0; P.out_status = (uint8_t*)dS.p + S.w0;
        P.sr_m = scores->sr_match; P.sr_n = scores->sr_mismatch; P.sr_g = scores->sr_gap;
        P.lr_m = scores->lr_match; P.lr_n = scores->lr_mismatch; P.lr_g = scores->lr_gap;
        P.n_arms = a1 - a0; P.draft4_bytes = d1 - d0; P.arms2_bytes = b1 - b0; P.flags = c.poa_flags;
        if ((e = hypo::poa_run(P, nw, dWS.p, wsb, c.num_cus, st, nullptr, &c.slots[0].aux)) != hipSuccess) return bad(HYPO_E_HIP, "poa_run", e);
        (void)hipMemcpyAsync(&S.st, (char*)dWS.p + 128, sizeof(HypoPoaStats), hipMemcpyDeviceToHost, st);
        if (!use_rccl) {                                   // results of this share straight back to the caller's buffers
            (void)hipMemcpyAsync(out->bases + out->off[S.w0], (char*)dB.p + out->off[S.w0], out->off[S.w1] - out->off[S.w0], hipMemcpyDeviceToHost, st);
            (void)hipMemcpyAsync(out->len + S.w0, (uint32_t*)dL.p + S.w0, (size_t)nw * 4, hipMemcpyDeviceToHost, st);
            (void)hipMemcpyAsync(out->status + S.w0, (uint8_t*)dS.p + S.w0, nw, hipMemcpyDeviceToHost, st);
            if ((e = hipStreamSynchronize(st)) != hipSuccess) return bad(HYPO_E_HIP, "hipStreamSynchronize", e);
        }
    };
    {
        std::vector<std::thread> th;
        for (int d = 0; d < nd; ++d) th.emplace_back(device_part, d);
        for (auto& t : th) t.join();
    }
    for (int d = 0; d < nd; ++d) if (sh[d].rc != HYPO_OK) return fail(sh[d].rc, "%s", sh[d].err);
    if (use_rccl) {
        // ---- 3. all-gatherv: owner r broadcasts its three ranges into the same places of every device's whole-batch buffers ----
        int r = g_rccl.GroupStart();
        for (int root = 0; r == 0 && root < nd; ++root) {
            const Share& S = sh[root];
            if (S.w1 == S.w0) continue;
            for (int d = 0; r == 0 && d < nd; ++d) {
                Ctx& c = g_ctxs[d];
                char* B = (char*)c.slots[0].arena[5].p; uint32_t* L = (uint32_t*)c.slots[0].arena[7].p; uint8_t* St = (uint8_t*)c.slots[0].arena[8].p;
                const size_t nb = out->off[S.w1] - out->off[S.w0], nw = S.w1 - S.w0;
                if (nb) r = g_rccl.Broadcast(B + out->off[S.w0], B + out->off[S.w0], nb, kNcclUint8, root, g_rccl.comms[d], c.stream);
                if (r == 0) r = g_rccl.Broadcast(L + S.w0, L + S.w0, nw * 4, kNcclUint8, root, g_rccl.comms[d], c.stream);
                if (r == 0) r = g_rccl.Broadcast(St + S.w0, St + S.w0, nw, kNcclUint8, root, g_rccl.comms[d], c.stream);
            }
        }
        const int r2 = g_rccl.GroupEnd();
        if (r != 0 || r2 != 0) return fail(HYPO_E_HIP, "RCCL all-gather of the consensus: %s", g_rccl.GetErrorString(r ? r : r2));
        // ---- 4. device 0 holds everything: one copy back for contig re-assembly; the other devices only have to finish ----
        Ctx& c0 = g_ctxs[0];
        HIP_TRY(hipSetDevice(c0.device));
        HIP_TRY(hipMemcpyAsync(out->bases, c0.slots[0].arena[5].p, out_bytes, hipMemcpyDeviceToHost, c0.stream));
        HIP_TRY(hipMemcpyAsync(out->len, c0.slots[0].arena[7].p, (size_t)n * 4, hipMemcpyDeviceToHost, c0.stream));
        HIP_TRY(hipMemcpyAsync(out->status, c0.slots[0].arena[8].p, n, hipMemcpyDeviceToHost, c0.stream));
        for (int d = nd - 1; d >= 0; --d) { HIP_TRY(hipSetDevice(g_ctxs[d].device)); HIP_TRY(hipStreamSynchronize(g_ctxs[d].stream)); }
    }
    HIP_TRY(hipSetDevice(g_ctx.device));
    for (int d = 0; d < nd; ++d) {
        const HypoPoaStats& s = sh[d].st;
        tl_stats.n_trivial += s.n_trivial; tl_stats.n_escalated += s.n_escalated; tl_stats.n_failed += s.n_failed;
        tl_stats.dp_cells += s.dp_cells; tl_stats.n_alignments += s.n_alignments;
        tl_stats.n_reused += s.n_reused; tl_stats.n_threaded += s.n_threaded; tl_stats.cells_scored += s.cells_scored; tl_stats.cells_threaded += s.cells_threaded; tl_stats.n_carried += s.n_carried;
        for (int k = 0; k < 8; ++k) { tl_stats.n_class[k] += s.n_class[k]; tl_stats.alg_bytes[k] += s.alg_bytes[k]; }
    }
    tl_stats.n_windows = n;
    return HYPO_OK;
}

// ---- solid scan ------------------------------------------------------------------------------------
size_t hypo_gpu_solid_scan_workspace_bytes(uint64_t n_bases) { return hypo::scan_workspace_bytes(n_bases); }

int hypo_gpu_solid_scan_device(const uint8_t* packed4, uint64_t n_bases, uint32_t k, const uint64_t* bits,
                               uint64_t* solid_pos_words, uint64_t* kids, uint64_t kids_cap,
                               uint64_t* word_rank, uint64_t* n_solid,
                               void* workspace, size_t workspace_bytes, void* hip_stream) {
    HYPO_ENTRY();
    if (const int rc = check_k(k)) return rc;
    if ((n_bases && !packed4) || !bits || (n_bases && !solid_pos_words)) return fail(HYPO_E_INVALID, "NULL buffer");
    if (!workspace || workspace_bytes < hypo::scan_workspace_bytes(n_bases))
        return fail(HYPO_E_WORKSPACE, "workspace %zu < required %zu", workspace_bytes, hypo::scan_workspace_bytes(n_bases));
    hipStream_t st = (hipStream_t)hip_stream;                  // NULL is the HIP null stream itself (what torch calls its default stream)
    ProfCall* pc = prof_next(2);
    if (pc) pc->ke.n = n_bases ? 4 : 0;                        // (an empty scan launches nothing: an empty record)
    HIP_TRY(hypo::scan_run(packed4, n_bases, k, bits, solid_pos_words, kids, kids_cap, word_rank, n_solid,
                           workspace, workspace_bytes, st, pc ? pc->ke.ev : nullptr));
    return HYPO_OK;
}

int hypo_gpu_solid_set_upload(const uint64_t* bits, uint32_t k) {
    HYPO_ENTRY();
    if (const int rc = check_k(k)) return rc;
    if (!bits) return fail(HYPO_E_INVALID, "NULL buffer");
    const uint64_t bit_words = (1ull << (2 * k)) / 64 ? (1ull << (2 * k)) / 64 : 1;
    g_ctx.solid_k = 0;
    HIP_TRY(g_ctx.solid_set.alloc(bit_words * 8));
    HIP_TRY(h2d(g_ctx.solid_set.p, bits, bit_words * 8, g_ctx.stream));
    HIP_TRY(hipStreamSynchronize(g_ctx.stream));
    g_ctx.solid_k = k;
    return HYPO_OK;
}

int hypo_gpu_solid_scan(const uint8_t* packed4, uint64_t n_bases, uint32_t k, const uint64_t* bits,
                        uint64_t* solid_pos_words, uint64_t* kids, uint64_t kids_cap,
                        uint64_t* word_rank, uint64_t* n_solid) {
    HYPO_ENTRY();
    if (const int rc = check_k(k)) return rc;
    if ((n_bases && !packed4) || (n_bases && !solid_pos_words)) return fail(HYPO_E_INVALID, "NULL buffer");
    if (!bits && g_ctx.solid_k != k) return fail(HYPO_E_INVALID, "bitset_words == NULL but no %u-mer set was uploaded (hypo_gpu_solid_set_upload)", k);
    const uint64_t nw = (n_bases + 63) / 64, nbytes = (n_bases + 1) / 2, bit_words = (1ull << (2 * k)) / 64 ? (1ull << (2 * k)) / 64 : 1;
    DevBuf* const sa = g_ctx.scan_arena;
    DevBuf &dP = sa[0], &dBits = sa[1], &dWords = sa[2], &dKids = sa[3], &dRank = sa[4], &dN = sa[5], &dWS = sa[6];
    const size_t wsb = hypo::scan_workspace_bytes(n_bases);
    HIP_TRY(dP.alloc(nbytes)); if (bits) HIP_TRY(dBits.alloc(bit_words * 8)); HIP_TRY(dWords.alloc(nw * 8));
    HIP_TRY(dKids.alloc(kids_cap * 8)); HIP_TRY(dRank.alloc((nw + 1) * 8)); HIP_TRY(dN.alloc(8)); HIP_TRY(dWS.alloc(wsb));
    hipStream_t st = g_ctx.stream;
    if (nbytes) HIP_TRY(h2d(dP.p, packed4, nbytes, st));
    if (bits) HIP_TRY(h2d(dBits.p, bits, bit_words * 8, st));
    int rc = hypo_gpu_solid_scan_device((const uint8_t*)dP.p, n_bases, k, (const uint64_t*)(bits ? dBits.p : g_ctx.solid_set.p), (uint64_t*)dWords.p,
                                        kids ? (uint64_t*)dKids.p : nullptr, kids ? kids_cap : 0, (uint64_t*)dRank.p,
                                        (uint64_t*)dN.p, dWS.p, wsb, st);
    if (rc) return rc;
    uint64_t ns = 0;
    HIP_TRY(hipMemcpyAsync(&ns, dN.p, 8, hipMemcpyDeviceToHost, st));
    if (nw) HIP_TRY(d2h(solid_pos_words, dWords.p, nw * 8, st));
    if (word_rank) HIP_TRY(d2h(word_rank, dRank.p, (nw + 1) * 8, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (kids && kids_cap) {
        const uint64_t cnt = ns < kids_cap ? ns : kids_cap;
        if (cnt) HIP_TRY(hipMemcpy(kids, dKids.p, cnt * 8, hipMemcpyDeviceToHost));
    }
    if (n_solid) *n_solid = ns;
    return HYPO_OK;
}

// ---- a scan whose k-mer ids and positions stay on the device (round 4) -------------------------------------------------------
// The host of a run needs the mark bits and their rank directory (Contig::_solid_pos); the k-mer ids and the positions are read
// by the support votes only, on the device: 8 bytes per marked position went to pageable host vectors here and came back, 12 per
// position with the positions, for hypo_gpu_support_kmers (2 x 2 GB at 250 Mbp / k = 15, where nearly every position is marked).
int hypo_gpu_solid_scan_keep(uint32_t handle, const uint8_t* packed4, uint64_t n_bases, uint32_t k,
                             uint64_t* solid_pos_words, uint64_t* word_rank, uint64_t* n_solid) {
    HYPO_ENTRY();
    if (const int rc = check_k(k)) return rc;
    if ((n_bases && !packed4) || (n_bases && !solid_pos_words)) return fail(HYPO_E_INVALID, "NULL buffer");
    if (g_ctx.solid_k != k) return fail(HYPO_E_INVALID, "no %u-mer set was uploaded (hypo_gpu_solid_set_upload)", k);
    if (handle >= (1u << 24) || n_bases >= 0xfffffff0ull) return fail(HYPO_E_INVALID, "handle or contig length out of range");
    const uint64_t nw = (n_bases + 63) / 64, nbytes = (n_bases + 1) / 2, cap = n_bases ? n_bases : 1;
    const bool narrow = k <= 16;
    DevBuf* const sa = g_ctx.scan_arena;
    DevBuf &dP = sa[0], &dWords = sa[2], &dKids = sa[3], &dRank = sa[4], &dN = sa[5], &dWS = sa[6];
    const size_t wsb = hypo::scan_workspace_bytes(n_bases);
    const size_t kid_bytes = narrow ? 4 : 8;
    HIP_TRY(dP.alloc(nbytes)); HIP_TRY(dWords.alloc(nw * 8)); HIP_TRY(dKids.alloc(cap * (kid_bytes + 4) + 256));
    HIP_TRY(dRank.alloc((nw + 1) * 8)); HIP_TRY(dN.alloc(8)); HIP_TRY(dWS.alloc(wsb));
    hipStream_t st = g_ctx.stream;
    char* const kid_arena = (char*)dKids.p;
    uint32_t* const spos_arena = (uint32_t*)(kid_arena + (cap * kid_bytes + 255) / 256 * 256);
    if (nbytes) HIP_TRY(h2d(dP.p, packed4, nbytes, st));
    HIP_TRY(hypo::scan_run((const uint8_t*)dP.p, n_bases, k, (const uint64_t*)g_ctx.solid_set.p, (uint64_t*)dWords.p,
                           narrow ? nullptr : (uint64_t*)kid_arena, cap, (uint64_t*)dRank.p, (uint64_t*)dN.p, dWS.p, wsb, st, nullptr,
                           narrow ? (uint32_t*)kid_arena : nullptr, spos_arena));
    uint64_t ns = 0;
    HIP_TRY(hipMemcpyAsync(&ns, dN.p, 8, hipMemcpyDeviceToHost, st));
    if (nw) HIP_TRY(d2h(solid_pos_words, dWords.p, nw * 8, st));
    if (word_rank) HIP_TRY(d2h(word_rank, dRank.p, (nw + 1) * 8, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (handle >= g_ctx.kept.size()) g_ctx.kept.resize((size_t)handle + 1);
    Ctx::KeptScan& ks = g_ctx.kept[handle];
    if (ks.kids) { (void)hipFree(ks.kids); ks.kids = nullptr; }
    if (ks.spos) { (void)hipFree(ks.spos); ks.spos = nullptr; }
    ks.used = false;
    if (ns) {
        HIP_TRY(hipMalloc(&ks.kids, ns * kid_bytes));
        HIP_TRY(hipMalloc((void**)&ks.spos, ns * 4));
        HIP_TRY(hipMemcpyAsync(ks.kids, kid_arena, ns * kid_bytes, hipMemcpyDeviceToDevice, st));      // (stream order keeps the arena
        HIP_TRY(hipMemcpyAsync(ks.spos, spos_arena, ns * 4, hipMemcpyDeviceToDevice, st));             //  intact until these ran)
    }
    ks.n = ns; ks.n_bases = n_bases; ks.k = k; ks.used = true;
    if (n_solid) *n_solid = ns;
    return HYPO_OK;
}

int hypo_gpu_solid_release(uint32_t handle) {
    HYPO_ENTRY();
    Ctx& cx = g_ctx;
    auto drop = [&cx](Ctx::KeptScan& ks) {
        const size_t kb = (size_t)ks.n * (ks.k <= 16 ? 4 : 8), sb = (size_t)ks.n * 4;
        if (ks.kids) { cx.kept_parked.push_back(ks.kids); cx.kept_parked_bytes += kb; }
        if (ks.spos) { cx.kept_parked.push_back(ks.spos); cx.kept_parked_bytes += sb; }
        ks = Ctx::KeptScan();
    };
    if (handle == 0xffffffffu) for (auto& ks : cx.kept) drop(ks);
    else {
        if (handle >= cx.kept.size() || !cx.kept[handle].used) return fail(HYPO_E_INVALID, "handle %u holds no scan on this context", handle);
        drop(cx.kept[handle]);
    }
    if (handle == 0xffffffffu || cx.kept_parked_bytes > ((size_t)16 << 30)) {
        HIP_TRY(hipStreamSynchronize(cx.stream));
        for (void* p : cx.kept_parked) (void)hipFree(p);
        cx.kept_parked.clear(); cx.kept_parked_bytes = 0;
    }
    return HYPO_OK;
}

// ---- the solid k-mer set from the short reads (kmer_kernel.hip; replaces KMC + suk::SolidKmers::initialise) --------------------
static constexpr uint64_t kKmerPiece = (uint64_t)256 << 20;     // bytes per kernel launch of hypo_gpu_kmer_count_add

int hypo_gpu_kmer_count_begin(uint32_t k, uint32_t coverage) {
    HYPO_ENTRY();
    if (k < 5 || k > 17) return fail(HYPO_E_INVALID, "k=%u out of range 5..17 (the count table holds 4^k counters: %.1f GiB at k = %u)",
                                     k, k <= 31 ? (double)(1ull << (2 * k)) / (1 << 30) : 0.0, k);
    if (coverage < 1 || coverage > HYPO_KMER_MAX_COVERAGE) return fail(HYPO_E_INVALID, "coverage %u out of range 1..%u", coverage, HYPO_KMER_MAX_COVERAGE);
    Ctx::KmerCount& kc = g_ctx.kc;
    if (kc.table) { (void)hipFree(kc.table); kc.table = nullptr; }
    kc.k = 0;
    kc.sat = 4 * coverage + 1;
    kc.wide = kc.sat > 255;
    kc.table_bytes = (size_t)(1ull << (2 * k)) * (kc.wide ? 2 : 1);
    hipError_t e = hipMalloc(&kc.table, kc.table_bytes);
    if (e != hipSuccess) { kc.table = nullptr; return fail(HYPO_E_HIP, "hipMalloc of the %.2f GiB count table (k = %u, %d-byte counters): %s",
                                                           (double)kc.table_bytes / (1 << 30), k, kc.wide ? 2 : 1, hipGetErrorString(e)); }
    HIP_TRY(kc.misc.alloc((size_t)(kc.sat + 2) * 8));
    HIP_TRY(hipMemsetAsync(kc.table, 0, kc.table_bytes, g_ctx.stream));
    HIP_TRY(hipStreamSynchronize(g_ctx.stream));
    kc.k = k; kc.cov = coverage;
    return HYPO_OK;
}

int hypo_gpu_kmer_count_add(const char* bytes, uint64_t n) {
    HYPO_ENTRY();
    Ctx::KmerCount& kc = g_ctx.kc;
    if (!kc.k) return fail(HYPO_E_INVALID, "no count table (hypo_gpu_kmer_count_begin)");
    if (!n) return HYPO_OK;
    if (!bytes) return fail(HYPO_E_INVALID, "NULL buffer");
    hipStream_t st = g_ctx.stream;
    HIP_TRY(kc.in.alloc(n < kKmerPiece ? n : kKmerPiece));
    // pieces of at most kKmerPiece bytes; each starts k - 1 bytes before the end of the one before, so that the k-mers that did
    // not end inside a piece are counted (once) by the next
    for (uint64_t at = 0;;) {
        const uint64_t m = n - at < kKmerPiece ? n - at : kKmerPiece;
        HIP_TRY(h2d(kc.in.p, bytes + at, m, st));
        HIP_TRY(hypo::kmer_count_run((const uint8_t*)kc.in.p, m, kc.k, kc.table, kc.wide, kc.sat, st));
        HIP_TRY(hipStreamSynchronize(st));                   // (the caller may refill `bytes` when this returns)
        if (at + m >= n) break;
        at += m - (kc.k - 1);
    }
    return HYPO_OK;
}

int hypo_gpu_kmer_histogram(uint64_t* hist, uint32_t n_bins) {
    HYPO_ENTRY();
    Ctx::KmerCount& kc = g_ctx.kc;
    if (!kc.k) return fail(HYPO_E_INVALID, "no count table (hypo_gpu_kmer_count_begin)");
    if (!hist || n_bins != 4 * kc.cov + 1) return fail(HYPO_E_INVALID, "hist needs 4c + 1 = %u bins (got %u)", 4 * kc.cov + 1, n_bins);
    hipStream_t st = g_ctx.stream;
    HIP_TRY(hypo::kmer_histogram_run(kc.table, kc.k, kc.wide, n_bins, (unsigned long long*)kc.misc.p, st));
    HIP_TRY(hipMemcpyAsync(hist, kc.misc.p, (size_t)n_bins * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return HYPO_OK;
}

int hypo_gpu_solid_set_build(uint32_t lower, uint32_t upper, int exclude_hp, uint64_t* bits, uint64_t* n_bits, uint64_t* n_canonical) {
    HYPO_ENTRY();
    Ctx::KmerCount& kc = g_ctx.kc;
    if (!kc.k) return fail(HYPO_E_INVALID, "no count table (hypo_gpu_kmer_count_begin)");
    if (!bits) return fail(HYPO_E_INVALID, "NULL buffer");
    hipStream_t st = g_ctx.stream;
    const uint64_t n_words = (1ull << (2 * kc.k)) / 64;
    // the set is written into the context's solid-set buffer: a later hypo_gpu_solid_set_upload of the same words re-fills it
    g_ctx.solid_k = 0;
    HIP_TRY(g_ctx.solid_set.alloc(n_words * 8));
    HIP_TRY(hypo::solid_fill_run(kc.table, kc.k, kc.wide, lower, upper, kc.sat, exclude_hp, (uint64_t*)g_ctx.solid_set.p,
                                 (unsigned long long*)kc.misc.p, st));
    uint64_t cnt[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(cnt, kc.misc.p, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(d2h(bits, g_ctx.solid_set.p, n_words * 8, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (n_bits) *n_bits = cnt[0];
    if (n_canonical) *n_canonical = cnt[1];
    return HYPO_OK;
}

int hypo_gpu_kmer_count_end(void) {
    HYPO_LOCKED();
    HYPO_ON_DEVICE();
    Ctx::KmerCount& kc = g_ctx.kc;
    if (kc.table) HIP_TRY(hipFree(kc.table));
    kc.in.release(); kc.misc.release();
    kc = Ctx::KmerCount();
    return HYPO_OK;
}

}  // extern "C"
// ---- the exact k-mer set of the reads (kset_kernel.hip; hypo --qv) -----------------------------------------------------------------
namespace {
double ks_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
uint64_t ks_slots_for(uint64_t keys) {                 // the smallest table that holds `keys` at KSET_MAX_LOAD
    const uint64_t s = (uint64_t)((double)keys / hypo::KSET_MAX_LOAD) + 1;
    return s < hypo::KSET_MIN_SLOTS ? hypo::KSET_MIN_SLOTS : s;
}
// The kernels' two counters: ks.ctr zeroed, launch(them on the device), both on their way down into ctr[].  The caller synchronises
// (an import has one more copy to queue first) and says what ctr[0] and the overflow flag ctr[1] mean to it.
template <class Launch>
hipError_t ks_counted(Ctx::KSet& ks, unsigned long long ctr[2], hipStream_t st, Launch launch) {
    hipError_t e = hipMemsetAsync(ks.ctr.p, 0, 16, st);
    if (e == hipSuccess) e = launch((unsigned long long*)ks.ctr.p);
    return e == hipSuccess ? hipMemcpyAsync(ctr, ks.ctr.p, 16, hipMemcpyDeviceToHost, st) : e;
}
// A fresh table of `slots` slots takes the keys of the present one (if any) and its place; with counts on, fresh planes beside it
// take the count bytes (the copy bytes are zero until the set is closed, and a closed set does not grow).
int ks_resize(Ctx::KSet& ks, uint64_t slots, hipStream_t st) {
    const double t0 = ks_now();
    uint64_t* fresh = nullptr;
    uint32_t* fresh_planes = nullptr;
    hipError_t e = hipMalloc((void**)&fresh, slots * 8);
    if (e == hipSuccess && ks.n_texts && (e = hipMalloc((void**)&fresh_planes, ks.plane_bytes(slots))) != hipSuccess) { (void)hipFree(fresh); fresh = nullptr; }
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(HYPO_E_HIP, "hipMalloc of a k-mer set table of %.3f GiB (%llu k-mers in the set): %s",
                                                                 (double)slots * ks.slot_bytes() / (1u << 30), (unsigned long long)ks.count, hipGetErrorString(e)); }
    auto drop = [&] { (void)hipFree(fresh); if (fresh_planes) (void)hipFree(fresh_planes); };
    unsigned long long ctr[2] = {0, 0};
    if ((e = hipMemsetAsync(fresh, 0xff, slots * 8, st)) == hipSuccess)
        e = ks_counted(ks, ctr, st, [&](unsigned long long* d_ctr) {
            const hipError_t z = fresh_planes ? hipMemsetAsync(fresh_planes, 0, ks.plane_bytes(slots), st) : hipSuccess;
            if (z != hipSuccess || !ks.table) return z;
            return ks.planes ? hypo::kset_rehash_count_run(ks.table, ks.slots, ks.planes, fresh, slots, fresh_planes, d_ctr, st)
                             : hypo::kset_rehash_run(ks.table, ks.slots, fresh, slots, d_ctr, st);
        });
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { drop(); return fail(HYPO_E_HIP, "k-mer set: resizing to %llu slots: %s", (unsigned long long)slots, hipGetErrorString(e)); }
    if (ctr[1] || ctr[0] != ks.count) {
        drop();
        return fail(HYPO_E_HIP, "k-mer set: internal error: %llu of %llu keys moved into %llu slots (overflow flag %llu)", ctr[0],
                    (unsigned long long)ks.count, (unsigned long long)slots, ctr[1]);
    }
    if (ks.table) { (void)hipFree(ks.table); ++ks.growths; ks.grow_s += ks_now() - t0; }
    if (ks.planes) (void)hipFree(ks.planes);
    ks.planes = fresh_planes;
    ks.table = fresh; ks.slots = slots;
    if (slots > ks.peak_slots) ks.peak_slots = slots;
    return HYPO_OK;
}
// Room for a call's worst case (every one of its `n_new` windows or records a new k-mer) is made before the table is touched: a call
// that cannot get it leaves the set as it was (HYPO_E_CAPACITY), and no kernel ever meets a table more than half full.
int ks_make_room(Ctx::KSet& ks, uint64_t n_new, const char* what, hipStream_t st) {
    const uint64_t worst = ks.count + n_new;
    const uint64_t need = ks_slots_for(worst);
    if (need <= ks.slots) return HYPO_OK;
    if (need > ks.max_slots)
        return fail(HYPO_E_CAPACITY, "the k-mer set holds %llu distinct %u-mers in a table of %.3f GiB; %llu more %s need %.3f GiB, the cap is %.3f GiB (--qv-mem)",
                    (unsigned long long)ks.count, ks.k, (double)ks.slots * ks.slot_bytes() / (1u << 30), (unsigned long long)n_new, what,
                    (double)need * ks.slot_bytes() / (1u << 30), (double)ks.max_slots * ks.slot_bytes() / (1u << 30));
    uint64_t slots = need > 2 * ks.slots ? need : 2 * ks.slots;
    if (slots > ks.max_slots) slots = ks.max_slots;
    return ks_resize(ks, slots, st);
}
// The entry points that need a live set: the lock, the device, `ks`.
#define HYPO_KSET_ENTRY() \
    HYPO_ENTRY(); \
    Ctx::KSet& ks = g_ctx.ks; \
    if (!ks.k) return fail(HYPO_E_INVALID, "no k-mer set (hypo_gpu_kset_begin)")
// Those that need its count bytes say so where the check stands in their order of checks.
#define KS_NEEDS_COUNTS() if (!ks.n_texts) return fail(HYPO_E_INVALID, "the k-mer set keeps no counts (hypo_gpu_kset_counts_enable)")
// [lo, hi) is a range of the call's n_bytes; `what` is the noun of the message, "span" or "site"
#define KS_CHECK_RANGE(what, s, lo, hi, n_bytes) \
    if ((lo) > (hi) || (hi) > (n_bytes)) \
        return fail(HYPO_E_INVALID, what " %u = [%llu, %llu) of %llu bytes", s, (unsigned long long)(lo), (unsigned long long)(hi), (unsigned long long)(n_bytes))

// The three arenas of a call as a Carver laid them out, on the context's stream: sized in the order in, off, res.
struct KsDev { DevAt in, off, res; };
int ks_arenas(Ctx::KSet& ks, size_t in_bytes, size_t off_bytes, size_t res_bytes, KsDev& d) {
    HIP_TRY(ks.in.alloc(in_bytes));
    HIP_TRY(ks.off.alloc(off_bytes));
    HIP_TRY(ks.res.alloc(res_bytes));
    d = {{(char*)ks.in.p, g_ctx.stream}, {(char*)ks.off.p, g_ctx.stream}, {(char*)ks.res.p, g_ctx.stream}};
    return HYPO_OK;
}

// rel[i] = off[i] - off[0], i = 0 .. n_seqs, of offsets that must not decrease
int ks_rel_offsets(const uint64_t* off, uint32_t n_seqs, std::vector<uint64_t>& rel) {
    rel.resize((size_t)n_seqs + 1);
    for (uint32_t i = 0; i <= n_seqs; ++i) {
        if (off[i] < off[0] || (i && off[i] < off[i - 1])) return fail(HYPO_E_INVALID, "off[] must not decrease (entry %u)", i);
        rel[i] = off[i] - off[0];
    }
    return HYPO_OK;
}

// What the two sequence queries and the mark do alike once their arguments are checked, for the n = rel.back() > 0 bytes at
// `bytes`: the arenas (ks.off of off_bytes, the offsets first; ks.res of n_sums pairs of sums), bytes and offsets up, zeroed sums,
// the caller's kernels through launch(the arenas, the sums).  The caller brings down what it wants and synchronises.
template <class Launch>
int ks_query_seqs(Ctx::KSet& ks, const char* bytes, const std::vector<uint64_t>& rel, size_t off_bytes, size_t n_sums, KsDev& d, Launch launch) {
    if (const int rc = ks_arenas(ks, rel.back(), off_bytes, n_sums * 16, d)) return rc;
    HIP_TRY(d.in.up(0, bytes, rel.back()));
    HIP_TRY(hipMemcpyAsync(d.off.base, rel.data(), rel.size() * 8, hipMemcpyHostToDevice, d.off.st));
    HIP_TRY(hipMemsetAsync(d.res.base, 0, n_sums * 16, d.res.st));
    HIP_TRY(launch(d, d.res.ull(0)));
    return HYPO_OK;
}

// What the two walk entries do alike before their kernel: the budget and the sites checked (the kernels trust what they are given),
// the arenas (ks.res of res_bytes), the text and from | to | dlo | dhi up; `sites` names them on the device.
int ks_walk_sites(Ctx::KSet& ks, const char* bytes, uint64_t n_bytes, const uint64_t* from, const uint64_t* to, const uint32_t* dlo, const uint32_t* dhi,
                  uint32_t n_sites, uint32_t budget, size_t res_bytes, KsDev& d, hypo::KsetWalkSites& sites) {
    const uint32_t k = ks.k;
    if (budget < 1 || budget > hypo::KSET_MAX_WALK_BUDGET) return fail(HYPO_E_INVALID, "budget = %u out of range 1..%u (HYPO_KSET_MAX_WALK_BUDGET)", budget, hypo::KSET_MAX_WALK_BUDGET);
    for (uint32_t s = 0; s < n_sites; ++s) {
        if (n_bytes < k || from[s] > n_bytes - k || to[s] > n_bytes - k)
            return fail(HYPO_E_INVALID, "site %u: the anchors at %llu and %llu (k = %u) do not lie inside %llu bytes", s, (unsigned long long)from[s], (unsigned long long)to[s], k,
                        (unsigned long long)n_bytes);
        if (dlo[s] < 1 || dlo[s] > dhi[s] || dhi[s] > hypo::KSET_MAX_WALK)
            return fail(HYPO_E_INVALID, "site %u: 1 <= dlo <= dhi <= %u (HYPO_KSET_MAX_WALK) does not hold for %u .. %u", s, hypo::KSET_MAX_WALK, dlo[s], dhi[s]);
    }
    Carver co;
    const size_t o_from = co.take((size_t)n_sites * 8), o_to = co.take((size_t)n_sites * 8), o_dlo = co.take((size_t)n_sites * 4), o_dhi = co.take((size_t)n_sites * 4);
    if (const int rc = ks_arenas(ks, n_bytes, co.at, res_bytes, d)) return rc;
    HIP_TRY(d.in.up(0, bytes, n_bytes));
    HIP_TRY(d.off.up(o_from, from, (size_t)n_sites * 8)); HIP_TRY(d.off.up(o_to, to, (size_t)n_sites * 8));
    HIP_TRY(d.off.up(o_dlo, dlo, (size_t)n_sites * 4)); HIP_TRY(d.off.up(o_dhi, dhi, (size_t)n_sites * 4));
    sites = {d.in.u8(0), d.off.u64(o_from), d.off.u64(o_to), d.off.u32(o_dlo), d.off.u32(o_dhi), n_sites};
    return HYPO_OK;
}
// Of a walk only its len bytes reach the caller: what lies beyond them in the caller's memory stays as it was.
void ks_walk_out(uint8_t* walk, const std::vector<uint8_t>& h_walk, size_t at, uint32_t len) {
    const size_t n = len <= hypo::KSET_MAX_WALK ? len : 0;
    for (size_t i = 0; i < n; ++i) walk[at * hypo::KSET_MAX_WALK + i] = h_walk[at * hypo::KSET_MAX_WALK + i];
}

// A run of n_win windows as pieces of at most KSET_SPAN_PIECE: f(first window, the piece's bytes), each piece with the k - 1 bytes
// its last window needs.
uint64_t ks_n_pieces(uint64_t n_win) { return (n_win + hypo::KSET_SPAN_PIECE - 1) / hypo::KSET_SPAN_PIECE; }
template <class F> void ks_pieces(uint64_t n_win, uint32_t k, F f) {
    for (uint64_t w = 0; w < n_win; w += hypo::KSET_SPAN_PIECE)
        f(w, (uint32_t)(n_win - w < hypo::KSET_SPAN_PIECE ? n_win - w : hypo::KSET_SPAN_PIECE) + k - 1);
}

int ks_group() {                                       // lanes per item; HYPO_KSET_SPAN_GROUP = 32 | 64 overrides (profiles/guard_rate.py)
    const char* g = getenv("HYPO_KSET_SPAN_GROUP");
    const int v = g ? atoi(g) : 0;
    return v == 64 || v == 32 ? v : hypo::KSET_SPAN_GROUP;
}
}  // namespace

extern "C" {

int hypo_gpu_kset_begin(uint32_t k, uint64_t expected_distinct, uint64_t max_bytes) {
    HYPO_ENTRY();
    if (k < 12 || k > 31) return fail(HYPO_E_INVALID, "k=%u out of range 12..31 (the key is the 2k-bit canonical code in a 64-bit slot)", k);
    if (!max_bytes) max_bytes = g_ctx.mem_free_at_init / 2;            // default cap: half of what the device had free at init
    const uint64_t max_slots = max_bytes / 8;
    if (max_slots < 2) return fail(HYPO_E_INVALID, "max_bytes = %llu holds no table", (unsigned long long)max_bytes);
    Ctx::KSet& ks = g_ctx.ks;
    if (ks.table) { (void)hipFree(ks.table); ks.table = nullptr; }
    if (ks.planes) { (void)hipFree(ks.planes); ks.planes = nullptr; }
    ks.k = 0; ks.slots = 0; ks.count = 0; ks.growths = 0; ks.grow_s = 0; ks.peak_slots = 0;
    ks.n_texts = 0; ks.marked = false; ks.min_count = 1;
    ks.max_slots = max_slots; ks.max_bytes = max_bytes;
    HIP_TRY(ks.ctr.alloc(16));
    uint64_t slots = ks_slots_for(expected_distinct < ((uint64_t)1 << 62) ? expected_distinct : ((uint64_t)1 << 62));
    if (slots > max_slots) slots = max_slots;
    const int rc = ks_resize(ks, slots, g_ctx.stream);
    if (rc != HYPO_OK) return rc;
    ks.k = k;
    return HYPO_OK;
}

int hypo_gpu_kset_add(const char* bytes, uint64_t n) {
    HYPO_KSET_ENTRY();
    if (ks.marked) return fail(HYPO_E_INVALID, "the k-mer set is closed: a text has been marked (hypo_gpu_kset_mark)");
    if (n < ks.k) return HYPO_OK;                                       // holds no k-mer
    if (!bytes) return fail(HYPO_E_INVALID, "NULL buffer");
    hipStream_t st = g_ctx.stream;
    if (const int rc = ks_make_room(ks, n - ks.k + 1, "windows", st)) return rc;
    HIP_TRY(ks.in.alloc(n < kKmerPiece ? n : kKmerPiece));
    // pieces as in hypo_gpu_kmer_count_add; a k-mer seen by two pieces is inserted twice, which changes nothing.  With counts on
    // every WINDOW must be in one piece only: consecutive pieces overlap by exactly k - 1 bytes (the step below), so a window lies
    // whole in the piece its first byte is new to, and inside a launch a lane owns the windows that start in its stretch.
    for (uint64_t at = 0;;) {
        const uint64_t m = n - at < kKmerPiece ? n - at : kKmerPiece;
        unsigned long long ctr[2] = {0, 0};
        HIP_TRY(h2d(ks.in.p, bytes + at, m, st));
        const hipError_t kset_insert = ks_counted(ks, ctr, st, [&](unsigned long long* d_ctr) {
            return ks.planes ? hypo::kset_insert_count_run((const uint8_t*)ks.in.p, m, ks.k, ks.table, ks.slots, d_ctr, ks.planes, st)
                             : hypo::kset_insert_run((const uint8_t*)ks.in.p, m, ks.k, ks.table, ks.slots, d_ctr, st);
        });
        HIP_TRY(kset_insert);
        HIP_TRY(hipStreamSynchronize(st));                   // (the caller may refill `bytes` when this returns)
        ks.count += ctr[0];
        if (ctr[1]) return fail(HYPO_E_HIP, "k-mer set: internal error: a table of %llu slots with %llu keys had no room", (unsigned long long)ks.slots, (unsigned long long)ks.count);
        if (at + m >= n) break;
        at += m - (ks.k - 1);
    }
    return HYPO_OK;
}

int hypo_gpu_kset_size(uint64_t* n_distinct, uint64_t* table_bytes) {
    HYPO_LOCKED();
    if (!g_ctx.ready) return fail(HYPO_E_NOTINIT, "hypo_gpu_init was not called");
    const Ctx::KSet& ks = g_ctx.ks;
    if (!ks.k) return fail(HYPO_E_INVALID, "no k-mer set (hypo_gpu_kset_begin)");
    if (n_distinct) *n_distinct = ks.count;
    if (table_bytes) *table_bytes = ks.slots * 8 + ks.plane_bytes(ks.slots);
    return HYPO_OK;
}

int hypo_gpu_kset_query(const char* bytes, const uint64_t* off, uint32_t n_seqs, uint64_t* total, uint64_t* missing) {
    HYPO_KSET_ENTRY();
    if (!n_seqs) return HYPO_OK;
    if (!off || !total || !missing) return fail(HYPO_E_INVALID, "NULL buffer");
    std::vector<uint64_t> rel;
    if (const int rc = ks_rel_offsets(off, n_seqs, rel)) return rc;
    for (uint32_t i = 0; i < n_seqs; ++i) total[i] = missing[i] = 0;
    if (!rel[n_seqs]) return HYPO_OK;
    if (!bytes) return fail(HYPO_E_INVALID, "NULL buffer");
    hipStream_t st = g_ctx.stream;
    KsDev d;
    if (const int rc = ks_query_seqs(ks, bytes + off[0], rel, rel.size() * 8, n_seqs, d, [&](const KsDev& a, unsigned long long* sums) {
            return hypo::kset_query_run(ks.view(), a.in.u8(0), a.off.u64(0), n_seqs, rel[n_seqs], sums, sums + n_seqs, st);
        })) return rc;
    HIP_TRY(hipMemcpyAsync(total, d.res.u64(0), (size_t)n_seqs * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(missing, d.res.u64(0) + n_seqs, (size_t)n_seqs * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return HYPO_OK;
}

int hypo_gpu_kset_query_track(const char* bytes, const uint64_t* off, uint32_t n_seqs, const uint8_t* want, uint64_t* total, uint64_t* missing,
                              uint64_t* iv_off, uint64_t* iv_start, uint64_t* iv_end, uint64_t* iv_missing, uint64_t iv_cap) {
    HYPO_KSET_ENTRY();
    if (iv_cap && (!iv_start || !iv_end || !iv_missing)) return fail(HYPO_E_INVALID, "NULL buffer");
    if (!n_seqs) { if (iv_off) iv_off[0] = 0; return HYPO_OK; }
    if (!off || !total || !missing || !iv_off) return fail(HYPO_E_INVALID, "NULL buffer");
    std::vector<uint64_t> rel;
    if (const int rc = ks_rel_offsets(off, n_seqs, rel)) return rc;
    const uint64_t n = rel[n_seqs];
    if (n && !bytes) return fail(HYPO_E_INVALID, "NULL buffer");
    for (uint32_t i = 0; i < n_seqs; ++i) total[i] = missing[i] = 0;
    for (uint32_t i = 0; i <= n_seqs; ++i) iv_off[i] = 0;
    if (!n) return HYPO_OK;
    hipStream_t st = g_ctx.stream;
    // `in`: the bytes.  `off`: the offsets, the want bytes, then what indexes the bytes: the two flag words per 32 positions, the
    // per-workgroup sums and their prefixes.  `res`: total / missing first.
    const uint32_t blocks = hypo::kset_track_blocks(n);
    const size_t n_words = (size_t)blocks * hypo::KS_THREADS;
    Carver co;
    co.take(rel.size() * 8);
    const size_t at_want = co.take(n_seqs), at_miss = co.take(n_words * 4), at_begin = co.take(n_words * 4), at_sums = co.take((size_t)blocks * 8),
                 at_pre = co.take(((size_t)blocks + 1) * 24);
    KsDev d;
    if (const int rc = ks_query_seqs(ks, bytes + off[0], rel, co.at, n_seqs, d, [&](const KsDev& a, unsigned long long* sums) {
            const DevAt& o = a.off;
            if (want) { const hipError_t e = hipMemcpyAsync(o.u8(at_want), want, n_seqs, hipMemcpyHostToDevice, st); if (e != hipSuccess) return e; }
            return hypo::kset_track_count_run(ks.view(), a.in.u8(0), o.u64(0), n_seqs, n, sums, sums + n_seqs, want ? o.u8(at_want) : nullptr, o.u32(at_miss),
                                              o.u32(at_begin), o.u64(at_sums), o.u64(at_pre), st);
        })) return rc;
    HIP_TRY(hipMemcpyAsync(total, d.res.u64(0), (size_t)n_seqs * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(missing, d.res.u64(0) + n_seqs, (size_t)n_seqs * 8, hipMemcpyDeviceToHost, st));
    const uint64_t* d_pre = d.off.u64(at_pre);
    uint64_t sums[3] = {0, 0, 0};                               // starts, ends, missing windows of the wanted sequences
    HIP_TRY(hipMemcpyAsync(sums, d_pre + 3 * (size_t)blocks, 24, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (sums[0] != sums[1]) return fail(HYPO_E_HIP, "k-mer track: internal error: %llu interval starts, %llu ends", (unsigned long long)sums[0], (unsigned long long)sums[1]);
    // total / missing and the number of intervals are on the host: `res` now takes iv_off and the intervals (a grown arena loses
    // nothing that is still needed)
    const uint64_t n_iv = sums[0];
    Carver cv;
    cv.take(rel.size() * 8);
    const size_t o_start = cv.take((size_t)n_iv * 8), o_end = cv.take((size_t)n_iv * 8), o_lo = cv.take((size_t)n_iv * 8), o_hi = cv.take((size_t)n_iv * 8);
    HIP_TRY(ks.res.alloc(cv.at));
    const DevAt r{(char*)ks.res.p, st};
    HIP_TRY(hypo::kset_track_emit_run(d.off.u64(0), n_seqs, n, ks.k, d.off.u32(at_miss), d.off.u32(at_begin), d_pre, n_iv, r.u64(0), r.u64(o_start), r.u64(o_end),
                                      r.u64(o_lo), r.u64(o_hi), st));
    HIP_TRY(hipMemcpyAsync(iv_off, r.base, rel.size() * 8, hipMemcpyDeviceToHost, st));
    const bool fits = n_iv <= iv_cap;
    if (fits) { HIP_TRY(r.down(iv_start, o_start, (size_t)n_iv * 8)); HIP_TRY(r.down(iv_end, o_end, (size_t)n_iv * 8)); HIP_TRY(r.down(iv_missing, o_hi, (size_t)n_iv * 8)); }
    HIP_TRY(hipStreamSynchronize(st));
    if (!fits) return fail(HYPO_E_WORKSPACE, "%llu intervals, room for %llu: call again with arrays of that size", (unsigned long long)n_iv, (unsigned long long)iv_cap);
    return HYPO_OK;
}

int hypo_gpu_kset_query_spans(const char* bytes, uint64_t n_bytes, const uint64_t* lo, const uint64_t* hi, uint32_t n_spans, uint64_t* total, uint64_t* missing) {
    HYPO_KSET_ENTRY();
    if (!n_spans) return HYPO_OK;
    if (!lo || !hi || !total || !missing) return fail(HYPO_E_INVALID, "NULL buffer");
    // a span longer than KSET_SPAN_PIECE windows becomes several items (each carries the k - 1 bytes its last window needs)
    const uint32_t k = ks.k;
    auto windows = [&](uint32_t s) { const uint64_t len = hi[s] - lo[s]; return len >= k ? len - k + 1 : 0; };
    uint64_t n_items = 0;
    for (uint32_t s = 0; s < n_spans; ++s) {
        KS_CHECK_RANGE("span", s, lo[s], hi[s], n_bytes);
        n_items += ks_n_pieces(windows(s));
    }
    for (uint32_t s = 0; s < n_spans; ++s) total[s] = missing[s] = 0;
    if (!n_items) return HYPO_OK;
    if (!bytes) return fail(HYPO_E_INVALID, "NULL buffer");
    if (n_items >= (1ull << 31)) return fail(HYPO_E_CAPACITY, "%llu pieces of spans in one call: split the call", (unsigned long long)n_items);
    std::vector<uint64_t> item_lo((size_t)n_items);
    std::vector<uint32_t> item_len((size_t)n_items);
    size_t it = 0;
    for (uint32_t s = 0; s < n_spans; ++s)
        ks_pieces(windows(s), k, [&](uint64_t w, uint32_t bytes_) { item_lo[it] = lo[s] + w; item_len[it++] = bytes_; });
    // ks.in: bytes.  ks.off: item_lo, then item_len at the next multiple of 256 bytes (the arena ends with it, unpadded).  ks.res: item pairs.
    hipStream_t st = g_ctx.stream;
    const size_t o_len = Carver::pad((size_t)n_items * 8);
    KsDev d;
    if (const int rc = ks_arenas(ks, n_bytes, o_len + (size_t)n_items * 4, (size_t)n_items * 8, d)) return rc;
    HIP_TRY(d.in.up(0, bytes, n_bytes));
    HIP_TRY(d.off.up(0, item_lo.data(), (size_t)n_items * 8)); HIP_TRY(d.off.up(o_len, item_len.data(), (size_t)n_items * 4));
    HIP_TRY(hypo::kset_spans_run(ks.view(), d.in.u8(0), d.off.u64(0), d.off.u32(o_len), (uint32_t)n_items, d.res.at<uint2>(0), ks_group(), st));
    std::vector<uint2> res((size_t)n_items);
    HIP_TRY(d.res.down(res.data(), 0, (size_t)n_items * 8));
    HIP_TRY(hipStreamSynchronize(st));
    it = 0;
    for (uint32_t s = 0; s < n_spans; ++s)
        for (uint64_t i = ks_n_pieces(windows(s)); i; --i, ++it) { total[s] += res[it].x; missing[s] += res[it].y; }
    return HYPO_OK;
}

int hypo_gpu_kset_query_variants(const char* bytes, uint64_t n_bytes, const char* alts, uint64_t n_alt_bytes, const uint64_t* lo, const uint64_t* hi,
                                 const uint32_t* edit_off, uint32_t n_sites, const uint64_t* eb, const uint64_t* ee, const uint64_t* ao, const uint32_t* al,
                                 uint32_t* best_mask, uint64_t* best_total, uint64_t* best_missing, uint64_t* var_total, uint64_t* var_missing) {
    HYPO_KSET_ENTRY();
    if (!n_sites) return HYPO_OK;
    if (!bytes || !lo || !hi || !edit_off || !best_mask || !best_total || !best_missing) return fail(HYPO_E_INVALID, "NULL buffer");
    // everything is checked before a buffer is touched: the kernels trust what they are given
    const uint32_t k = ks.k;
    const uint32_t e_first = edit_off[0];
    uint64_t n_vars = 0, n_items = 0;
    for (uint32_t s = 0; s < n_sites; ++s) {
        if (edit_off[s + 1] < edit_off[s]) return fail(HYPO_E_INVALID, "edit_off[] must not decrease (entry %u)", s + 1);
        const uint32_t n = edit_off[s + 1] - edit_off[s];
        if (n > hypo::KSET_MAX_EDITS) return fail(HYPO_E_INVALID, "site %u has %u edits, at most %u (HYPO_KSET_MAX_EDITS)", s, n, hypo::KSET_MAX_EDITS);
        KS_CHECK_RANGE("site", s, lo[s], hi[s], n_bytes);
        if (n && (!eb || !ee || !ao || !al)) return fail(HYPO_E_INVALID, "NULL buffer");
        uint64_t at = lo[s], longest = hi[s] - lo[s];
        for (uint32_t e = edit_off[s]; e < edit_off[s + 1]; ++e) {
            if (eb[e] < at || ee[e] < eb[e] || ee[e] > hi[s])
                return fail(HYPO_E_INVALID, "edit %u of site %u = [%llu, %llu): the edits of a site ascend, do not overlap and stay inside [%llu, %llu)", e - edit_off[s], s,
                            (unsigned long long)eb[e], (unsigned long long)ee[e], (unsigned long long)lo[s], (unsigned long long)hi[s]);
            if (ao[e] > n_alt_bytes || al[e] > n_alt_bytes - ao[e] || (al[e] && !alts))
                return fail(HYPO_E_INVALID, "edit %u of site %u: ALT [%llu, +%u) of %llu bytes", e - edit_off[s], s, (unsigned long long)ao[e], al[e], (unsigned long long)n_alt_bytes);
            at = ee[e];
            longest += al[e];
        }
        if (longest >= (1ull << 31)) return fail(HYPO_E_INVALID, "site %u: a variant of %llu bytes (at most 2^31 - 1)", s, (unsigned long long)longest);
        n_vars += 1ull << n;
        if (n_vars > 0xffffffffull) return fail(HYPO_E_INVALID, "more than 2^32 - 1 variants in one call (site %u): split the call", s);
    }
    // the items: every variant at least one, a variant with more than KSET_SPAN_PIECE windows several (each carries the k - 1 bytes
    // its last window needs)
    std::vector<uint4> items;
    std::vector<uint32_t> site_item((size_t)n_sites + 1), var_off((size_t)n_sites + 1), rel_off((size_t)n_sites + 1);
    items.reserve((size_t)(n_vars < (1u << 24) ? n_vars : (1u << 24)));
    uint64_t vars_before = 0;
    for (uint32_t s = 0; s < n_sites; ++s) {
        const uint32_t e0 = edit_off[s], n = edit_off[s + 1] - e0;
        site_item[s] = (uint32_t)items.size(); var_off[s] = (uint32_t)vars_before; rel_off[s] = e0 - e_first;
        const int64_t base = (int64_t)(hi[s] - lo[s]);
        for (uint32_t m = 0; m < (1u << n); ++m) {
            int64_t len = base;
            for (uint32_t j = 0; j < n; ++j) if ((m >> j) & 1u) len += (int64_t)al[e0 + j] - (int64_t)(ee[e0 + j] - eb[e0 + j]);
            const uint32_t n_win = len >= (int64_t)k ? (uint32_t)len - k + 1 : 0;
            if (!n_win) items.push_back(make_uint4(s, m, 0, 0));
            ks_pieces(n_win, k, [&](uint64_t w, uint32_t bytes_) { items.push_back(make_uint4(s, m, (uint32_t)w, bytes_)); });
        }
        vars_before += 1ull << n;
        if (items.size() >= (1ull << 31)) return fail(HYPO_E_CAPACITY, "%llu pieces of variants in one call: split the call", (unsigned long long)items.size());
    }
    site_item[n_sites] = (uint32_t)items.size(); var_off[n_sites] = (uint32_t)n_vars; rel_off[n_sites] = edit_off[n_sites] - e_first;
    n_items = items.size();
    const uint32_t n_edits = edit_off[n_sites] - e_first;
    const bool want_vars = var_total || var_missing;
    hipStream_t st = g_ctx.stream;
    // ks.in: bytes | alts.  ks.off: site_lo | eb | ee | ao | items | edit_off | al | site_item | var_off.  ks.res: item pairs |
    // best_total | best_missing | var_total | var_missing | best_mask.  Every section starts at a multiple of 256 bytes.
    const size_t alt_at = Carver::pad((size_t)n_bytes);
    Carver co, cr;
    const size_t o_lo = co.take((size_t)n_sites * 8), o_eb = co.take((size_t)n_edits * 8), o_ee = co.take((size_t)n_edits * 8), o_ao = co.take((size_t)n_edits * 8),
                 o_items = co.take((size_t)n_items * 16), o_eoff = co.take(((size_t)n_sites + 1) * 4), o_al = co.take((size_t)n_edits * 4),
                 o_sitem = co.take(((size_t)n_sites + 1) * 4), o_voff = co.take(((size_t)n_sites + 1) * 4);
    const size_t r_item = cr.take((size_t)n_items * 8), r_bt = cr.take((size_t)n_sites * 8), r_bm = cr.take((size_t)n_sites * 8),
                 r_vt = cr.take(want_vars ? (size_t)n_vars * 8 : 0), r_vm = cr.take(want_vars ? (size_t)n_vars * 8 : 0), r_mask = cr.take((size_t)n_sites * 4);
    KsDev d;
    if (const int rc = ks_arenas(ks, alt_at + (size_t)n_alt_bytes, co.at, cr.at, d)) return rc;
    HIP_TRY(d.in.up(0, bytes, n_bytes)); HIP_TRY(d.in.up(alt_at, alts, n_alt_bytes));
    HIP_TRY(d.off.up(o_lo, lo, (size_t)n_sites * 8));
    if (n_edits) {                                              // (with no edit the four arrays may be NULL)
        HIP_TRY(d.off.up(o_eb, eb + e_first, (size_t)n_edits * 8)); HIP_TRY(d.off.up(o_ee, ee + e_first, (size_t)n_edits * 8));
        HIP_TRY(d.off.up(o_ao, ao + e_first, (size_t)n_edits * 8)); HIP_TRY(d.off.up(o_al, al + e_first, (size_t)n_edits * 4));
    }
    HIP_TRY(d.off.up(o_items, items.data(), (size_t)n_items * 16)); HIP_TRY(d.off.up(o_eoff, rel_off.data(), rel_off.size() * 4));
    HIP_TRY(d.off.up(o_sitem, site_item.data(), site_item.size() * 4)); HIP_TRY(d.off.up(o_voff, var_off.data(), var_off.size() * 4));
    const hypo::KsetVariantsIn in{d.in.u8(0), d.in.u8(alt_at), d.off.u64(o_lo), d.off.u32(o_eoff), d.off.u64(o_eb), d.off.u64(o_ee), d.off.u64(o_ao), d.off.u32(o_al),
                                  d.off.at<uint4>(o_items), (uint32_t)n_items, d.off.u32(o_sitem), d.off.u32(o_voff), n_sites};
    const hypo::KsetVariantsOut out{d.res.at<uint2>(r_item), d.res.u32(r_mask), d.res.ull(r_bt), d.res.ull(r_bm), want_vars ? d.res.ull(r_vt) : nullptr,
                                    want_vars ? d.res.ull(r_vm) : nullptr};
    HIP_TRY(hypo::kset_variants_run(ks.view(), in, out, ks_group(), st));
    HIP_TRY(d.res.down(best_mask, r_mask, (size_t)n_sites * 4));
    HIP_TRY(d.res.down(best_total, r_bt, (size_t)n_sites * 8)); HIP_TRY(d.res.down(best_missing, r_bm, (size_t)n_sites * 8));
    if (var_total) HIP_TRY(d.res.down(var_total, r_vt, (size_t)n_vars * 8));
    if (var_missing) HIP_TRY(d.res.down(var_missing, r_vm, (size_t)n_vars * 8));
    HIP_TRY(hipStreamSynchronize(st));
    return HYPO_OK;
}

int hypo_gpu_kset_query_fixes(const char* bytes, uint64_t n_bytes, const uint64_t* lo, const uint64_t* hi, const uint64_t* c0, const uint64_t* c1, uint32_t n_sites,
                              uint64_t* none_total, uint64_t* none_missing, uint32_t* best_cand, uint64_t* best_total, uint64_t* best_missing, uint32_t* zeros,
                              uint64_t* cand_total, uint64_t* cand_missing) {
    HYPO_KSET_ENTRY();
    if (!n_sites) return HYPO_OK;
    if (!bytes || !lo || !hi || !c0 || !c1 || !none_total || !none_missing || !best_cand || !best_total || !best_missing || !zeros) return fail(HYPO_E_INVALID, "NULL buffer");
    if (!cand_total != !cand_missing) return fail(HYPO_E_INVALID, "cand_total and cand_missing are both given or both NULL");
    static_assert(hypo::KSET_MAX_FIX_REGION == HYPO_KSET_MAX_FIX_REGION && hypo::KSET_MAX_FIX_SPAN == HYPO_KSET_MAX_FIX_SPAN, "the header's limits");
    // everything is checked before a buffer is touched: the kernels trust what they are given
    std::vector<uint32_t> len(n_sites), rc0(n_sites), w(n_sites), item_off((size_t)n_sites + 1);
    uint64_t n_items = 0;
    for (uint32_t s = 0; s < n_sites; ++s) {
        if (!(lo[s] <= c0[s] && c0[s] < c1[s] && c1[s] <= hi[s] && hi[s] <= n_bytes))
            return fail(HYPO_E_INVALID, "site %u: lo <= c0 < c1 <= hi <= n_bytes does not hold for [%llu, %llu) with the region [%llu, %llu) of %llu bytes", s,
                        (unsigned long long)lo[s], (unsigned long long)hi[s], (unsigned long long)c0[s], (unsigned long long)c1[s], (unsigned long long)n_bytes);
        if (c1[s] - c0[s] > hypo::KSET_MAX_FIX_REGION) return fail(HYPO_E_INVALID, "site %u: a region of %llu bytes, at most %u (HYPO_KSET_MAX_FIX_REGION)", s, (unsigned long long)(c1[s] - c0[s]), hypo::KSET_MAX_FIX_REGION);
        if (hi[s] - lo[s] > hypo::KSET_MAX_FIX_SPAN) return fail(HYPO_E_INVALID, "site %u: a span of %llu bytes, at most %u (HYPO_KSET_MAX_FIX_SPAN)", s, (unsigned long long)(hi[s] - lo[s]), hypo::KSET_MAX_FIX_SPAN);
        len[s] = (uint32_t)(hi[s] - lo[s]); rc0[s] = (uint32_t)(c0[s] - lo[s]); w[s] = (uint32_t)(c1[s] - c0[s]);
        item_off[s] = (uint32_t)n_items;
        n_items += 9ull * w[s] - 3;
        if (n_items >= (1ull << 31)) return fail(HYPO_E_CAPACITY, "%llu candidates in one call (site %u): split the call", (unsigned long long)n_items, s);
    }
    item_off[n_sites] = (uint32_t)n_items;
    const bool want_cands = cand_total != nullptr;
    hipStream_t st = g_ctx.stream;
    // ks.in: bytes.  ks.off: site_lo | site_len | site_c0 | site_w | item_off.  ks.res: item pairs | none_total | none_missing |
    // best_total | best_missing | cand_total | cand_missing | best_cand | zeros.  Every section starts at a multiple of 256 bytes.
    Carver co, cr;
    const size_t o_lo = co.take((size_t)n_sites * 8), o_len = co.take((size_t)n_sites * 4), o_c0 = co.take((size_t)n_sites * 4), o_w = co.take((size_t)n_sites * 4),
                 o_ioff = co.take(((size_t)n_sites + 1) * 4);
    const size_t r_item = cr.take((size_t)n_items * 8), r_nt = cr.take((size_t)n_sites * 8), r_nm = cr.take((size_t)n_sites * 8), r_bt = cr.take((size_t)n_sites * 8),
                 r_bm = cr.take((size_t)n_sites * 8), r_ct = cr.take(want_cands ? (size_t)n_items * 8 : 0), r_cm = cr.take(want_cands ? (size_t)n_items * 8 : 0),
                 r_bc = cr.take((size_t)n_sites * 4), r_z = cr.take((size_t)n_sites * 4);
    KsDev d;
    if (const int rc = ks_arenas(ks, n_bytes, co.at, cr.at, d)) return rc;
    HIP_TRY(d.in.up(0, bytes, n_bytes)); HIP_TRY(d.off.up(o_lo, lo, (size_t)n_sites * 8));
    HIP_TRY(d.off.up(o_len, len.data(), (size_t)n_sites * 4)); HIP_TRY(d.off.up(o_c0, rc0.data(), (size_t)n_sites * 4));
    HIP_TRY(d.off.up(o_w, w.data(), (size_t)n_sites * 4)); HIP_TRY(d.off.up(o_ioff, item_off.data(), item_off.size() * 4));
    const hypo::KsetFixesIn in{d.in.u8(0), d.off.u64(o_lo), d.off.u32(o_len), d.off.u32(o_c0), d.off.u32(o_w), d.off.u32(o_ioff), n_sites, (uint32_t)n_items};
    const hypo::KsetFixesOut out{d.res.at<uint2>(r_item), d.res.ull(r_nt), d.res.ull(r_nm), d.res.u32(r_bc), d.res.ull(r_bt), d.res.ull(r_bm), d.res.u32(r_z),
                                 want_cands ? d.res.ull(r_ct) : nullptr, want_cands ? d.res.ull(r_cm) : nullptr};
    HIP_TRY(hypo::kset_fixes_run(ks.view(), in, out, ks_group(), st));
    HIP_TRY(d.res.down(none_total, r_nt, (size_t)n_sites * 8)); HIP_TRY(d.res.down(none_missing, r_nm, (size_t)n_sites * 8));
    HIP_TRY(d.res.down(best_cand, r_bc, (size_t)n_sites * 4));
    HIP_TRY(d.res.down(best_total, r_bt, (size_t)n_sites * 8)); HIP_TRY(d.res.down(best_missing, r_bm, (size_t)n_sites * 8));
    HIP_TRY(d.res.down(zeros, r_z, (size_t)n_sites * 4));
    if (want_cands) { HIP_TRY(d.res.down(cand_total, r_ct, (size_t)n_items * 8)); HIP_TRY(d.res.down(cand_missing, r_cm, (size_t)n_items * 8)); }
    HIP_TRY(hipStreamSynchronize(st));
    return HYPO_OK;
}

int hypo_gpu_kset_query_walks(const char* bytes, uint64_t n_bytes, const uint64_t* from, const uint64_t* to, const uint32_t* dlo, const uint32_t* dhi,
                              uint32_t n_sites, uint32_t budget, uint32_t* status, uint32_t* steps, uint32_t* len, uint8_t* walk) {
    HYPO_KSET_ENTRY();
    if (!n_sites) return HYPO_OK;
    if (!bytes || !from || !to || !dlo || !dhi || !status || !steps || !len || !walk) return fail(HYPO_E_INVALID, "NULL buffer");
    static_assert(hypo::KSET_MAX_WALK == HYPO_KSET_MAX_WALK && hypo::KSET_MAX_WALK_BUDGET == HYPO_KSET_MAX_WALK_BUDGET, "the header's limits");
    hipStream_t st = g_ctx.stream;
    // ks.in: bytes.  ks.off: from | to | dlo | dhi.  ks.res: status | steps | len | walk.  Every section starts at a multiple of 256 bytes.
    Carver cr;
    const size_t r_st = cr.take((size_t)n_sites * 4), r_steps = cr.take((size_t)n_sites * 4), r_len = cr.take((size_t)n_sites * 4),
                 r_walk = cr.take((size_t)n_sites * hypo::KSET_MAX_WALK);
    KsDev d;
    hypo::KsetWalkSites sites;
    if (const int rc = ks_walk_sites(ks, bytes, n_bytes, from, to, dlo, dhi, n_sites, budget, cr.at, d, sites)) return rc;
    HIP_TRY(hypo::kset_walks_run(ks.view(), sites, budget, d.res.u32(r_st), d.res.u32(r_steps), d.res.u32(r_len), d.res.u8(r_walk), st));
    // through host buffers of the call's own: of a walk only its len bytes reach the caller, what lies beyond them stays as it was
    std::vector<uint32_t> h_st(n_sites), h_steps(n_sites), h_len(n_sites);
    std::vector<uint8_t> h_walk((size_t)n_sites * hypo::KSET_MAX_WALK);
    HIP_TRY(d.res.down(h_st.data(), r_st, (size_t)n_sites * 4)); HIP_TRY(d.res.down(h_steps.data(), r_steps, (size_t)n_sites * 4));
    HIP_TRY(d.res.down(h_len.data(), r_len, (size_t)n_sites * 4)); HIP_TRY(d.res.down(h_walk.data(), r_walk, h_walk.size()));
    HIP_TRY(hipStreamSynchronize(st));
    for (uint32_t s = 0; s < n_sites; ++s) {
        status[s] = h_st[s]; steps[s] = h_steps[s]; len[s] = h_len[s];
        ks_walk_out(walk, h_walk, s, h_len[s]);
    }
    return HYPO_OK;
}

int hypo_gpu_kset_query_walk_sets(const char* bytes, uint64_t n_bytes, const uint64_t* from, const uint64_t* to, const uint32_t* dlo, const uint32_t* dhi,
                                  uint32_t n_sites, uint32_t budget, uint32_t* status, uint32_t* steps, uint32_t* n_walks, uint32_t* len, uint32_t* low,
                                  uint8_t* walk) {
    HYPO_KSET_ENTRY();
    if (!n_sites) return HYPO_OK;
    if (!bytes || !from || !to || !dlo || !dhi || !status || !steps || !n_walks || !len || !low || !walk) return fail(HYPO_E_INVALID, "NULL buffer");
    static_assert(hypo::KSET_WALK_SETS == HYPO_KSET_MAX_WALKS, "the header's limits");
    KS_NEEDS_COUNTS();
    constexpr size_t W = hypo::KSET_WALK_SETS, MW = hypo::KSET_MAX_WALK;
    hipStream_t st = g_ctx.stream;
    // ks.in: bytes.  ks.off: from | to | dlo | dhi.  ks.res: status | steps | n_walks | len | low | walk.  Every section starts at a multiple of 256 bytes.
    Carver cr;
    const size_t r_st = cr.take((size_t)n_sites * 4), r_steps = cr.take((size_t)n_sites * 4), r_nw = cr.take((size_t)n_sites * 4), r_len = cr.take((size_t)n_sites * W * 4),
                 r_low = cr.take((size_t)n_sites * W * 4), r_walk = cr.take((size_t)n_sites * W * MW);
    KsDev d;
    hypo::KsetWalkSites sites;
    if (const int rc = ks_walk_sites(ks, bytes, n_bytes, from, to, dlo, dhi, n_sites, budget, cr.at, d, sites)) return rc;
    HIP_TRY(hypo::kset_walk_sets_run(ks.view(), sites, budget, d.res.u32(r_st), d.res.u32(r_steps), d.res.u32(r_nw), d.res.u32(r_len), d.res.u32(r_low), d.res.u8(r_walk), st));
    // through host buffers of the call's own: only the slots below n_walks and of a walk only its len bytes reach the caller, what lies
    // beyond them stays as it was (the arena is not cleared: a slot the search did not fill holds an earlier call's bytes)
    std::vector<uint32_t> h_st(n_sites), h_steps(n_sites), h_nw(n_sites), h_len(n_sites * W), h_low(n_sites * W);
    std::vector<uint8_t> h_walk((size_t)n_sites * W * MW);
    HIP_TRY(d.res.down(h_st.data(), r_st, (size_t)n_sites * 4)); HIP_TRY(d.res.down(h_steps.data(), r_steps, (size_t)n_sites * 4));
    HIP_TRY(d.res.down(h_nw.data(), r_nw, (size_t)n_sites * 4)); HIP_TRY(d.res.down(h_len.data(), r_len, h_len.size() * 4));
    HIP_TRY(d.res.down(h_low.data(), r_low, h_low.size() * 4)); HIP_TRY(d.res.down(h_walk.data(), r_walk, h_walk.size()));
    HIP_TRY(hipStreamSynchronize(st));
    for (uint32_t s = 0; s < n_sites; ++s) {
        status[s] = h_st[s]; steps[s] = h_steps[s]; n_walks[s] = h_nw[s];
        const size_t nw = h_nw[s] <= W ? h_nw[s] : 0;
        for (size_t w = 0; w < nw; ++w) {
            const size_t at = (size_t)s * W + w;
            len[at] = h_len[at]; low[at] = h_low[at];
            ks_walk_out(walk, h_walk, at, h_len[at]);
        }
    }
    return HYPO_OK;
}

// ---- read counts, copy numbers and the spectrum (hypo --qv-spectra) ---------------------------------------------------------------
int hypo_gpu_kset_counts_enable(uint32_t n_texts) {
    HYPO_KSET_ENTRY();
    if (n_texts < 1 || n_texts > hypo::KSET_MAX_TEXTS) return fail(HYPO_E_INVALID, "n_texts = %u out of range 1..%u", n_texts, hypo::KSET_MAX_TEXTS);
    if (ks.n_texts) return fail(HYPO_E_INVALID, "the k-mer set counts already");
    if (ks.count) return fail(HYPO_E_INVALID, "the k-mer set holds %llu k-mers: counts are enabled while it is empty, right after hypo_gpu_kset_begin", (unsigned long long)ks.count);
    const uint64_t max_slots = ks.max_bytes / (9 + n_texts);
    if (max_slots < 2) return fail(HYPO_E_INVALID, "max_bytes = %llu holds no table with counts", (unsigned long long)ks.max_bytes);
    // the (empty) table is replaced by one with its planes beside it, smaller when the cap of 9 + n_texts bytes a slot asks for it
    const uint64_t was_max = ks.max_slots;
    const uint32_t growths = ks.growths;
    const double grow_s = ks.grow_s;
    ks.n_texts = n_texts; ks.max_slots = max_slots;
    const int rc = ks_resize(ks, ks.slots < max_slots ? ks.slots : max_slots, g_ctx.stream);
    if (rc != HYPO_OK) { ks.n_texts = 0; ks.max_slots = was_max; return rc; }
    ks.growths = growths; ks.grow_s = grow_s;                          // (nothing was moved)
    return HYPO_OK;
}

int hypo_gpu_kset_mark(uint32_t text, const char* bytes, const uint64_t* off, uint32_t n_seqs, uint64_t* n_windows, uint64_t* n_unmarked) {
    HYPO_KSET_ENTRY();
    KS_NEEDS_COUNTS();
    if (text >= ks.n_texts) return fail(HYPO_E_INVALID, "text = %u, the set has %u", text, ks.n_texts);
    std::vector<uint64_t> rel(1, 0);
    if (n_seqs) {
        if (!off) return fail(HYPO_E_INVALID, "NULL buffer");
        if (const int rc = ks_rel_offsets(off, n_seqs, rel)) return rc;
        if (rel[n_seqs] && !bytes) return fail(HYPO_E_INVALID, "NULL buffer");
    }
    ks.marked = true;                                                  // from here on the copy bytes may be other than zero
    unsigned long long sums[2] = {0, 0};
    if (rel.back()) {                                                  // one pair of sums for the whole text
        hipStream_t st = g_ctx.stream;
        KsDev d;
        if (const int rc = ks_query_seqs(ks, bytes + off[0], rel, rel.size() * 8, 1, d, [&](const KsDev& a, unsigned long long* d_sums) {
                return hypo::kset_mark_run(a.in.u8(0), a.off.u64(0), n_seqs, rel.back(), ks.k, ks.table, ks.slots, ks.planes, text, d_sums, st);
            })) return rc;
        HIP_TRY(hipMemcpyAsync(sums, d.res.base, 16, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    if (n_windows) *n_windows = sums[0];
    if (n_unmarked) *n_unmarked = sums[1];
    return HYPO_OK;
}

int hypo_gpu_kset_spectrum(uint32_t text, uint64_t* hist) {
    HYPO_KSET_ENTRY();
    KS_NEEDS_COUNTS();
    if (text >= ks.n_texts) return fail(HYPO_E_INVALID, "text = %u, the set has %u", text, ks.n_texts);
    if (!hist) return fail(HYPO_E_INVALID, "NULL buffer");
    hipStream_t st = g_ctx.stream;
    constexpr size_t kBytes = (size_t)hypo::KSET_HIST_BINS * 8;
    static_assert(hypo::KSET_HIST_BINS == HYPO_KSET_SPECTRUM_BINS, "the header's size of hist[]");
    HIP_TRY(ks.res.alloc(kBytes));
    HIP_TRY(hipMemsetAsync(ks.res.p, 0, kBytes, st));
    HIP_TRY(hypo::kset_spectrum_run(ks.planes, ks.slots, text, (unsigned long long*)ks.res.p, st));
    HIP_TRY(hipMemcpyAsync(hist, ks.res.p, kBytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return HYPO_OK;
}

// ---- a least count for the queries (hypo --qv-min-count) --------------------------------------------------------------------------
int hypo_gpu_kset_min_count(uint32_t t) {
    HYPO_KSET_ENTRY();
    KS_NEEDS_COUNTS();
    if (t < 1 || t > 255) return fail(HYPO_E_INVALID, "t = %u out of range 1..255 (the k-mer set counts up to 255)", t);
    ks.min_count = t;                                                  // read when a query launches: the counts are those of that moment
    return HYPO_OK;
}

// ---- read count against copy number per bin (hypo --qv-cn) -------------------------------------------------------------------------
// Arenas: ks.in the bytes; ks.off the offsets and, behind them, the bin offsets; ks.res the six arrays.  The kernel writes every
// entry below n_bins, so nothing is cleared and nothing of the caller's is touched before the results are down.
int hypo_gpu_kset_query_depth(const char* bytes, const uint64_t* off, uint32_t n_seqs, uint32_t bin, uint32_t text, uint32_t unit, uint64_t n_bins,
                              uint32_t* windows, uint32_t* missing, uint32_t* rated, uint32_t* over, uint32_t* under, uint8_t* med_count) {
    HYPO_KSET_ENTRY();
    KS_NEEDS_COUNTS();
    static_assert(hypo::KSET_DEPTH_MIN_BIN == HYPO_KSET_DEPTH_MIN_BIN && hypo::KSET_DEPTH_MAX_BIN == HYPO_KSET_DEPTH_MAX_BIN, "the header's range of bin");
    if (text >= ks.n_texts) return fail(HYPO_E_INVALID, "text = %u, the set has %u", text, ks.n_texts);
    if (bin < hypo::KSET_DEPTH_MIN_BIN || bin > hypo::KSET_DEPTH_MAX_BIN)
        return fail(HYPO_E_INVALID, "bin = %u out of range %u..%u (HYPO_KSET_DEPTH_MIN_BIN, HYPO_KSET_DEPTH_MAX_BIN)", bin, hypo::KSET_DEPTH_MIN_BIN, hypo::KSET_DEPTH_MAX_BIN);
    if (unit < 1 || unit > 255) return fail(HYPO_E_INVALID, "unit = %u out of range 1..255 (the k-mer set counts up to 255)", unit);
    if (!n_seqs) return n_bins ? fail(HYPO_E_INVALID, "n_bins = %llu, no sequence has a bin", (unsigned long long)n_bins) : HYPO_OK;
    if (!off) return fail(HYPO_E_INVALID, "NULL buffer");
    std::vector<uint64_t> rel;
    if (const int rc = ks_rel_offsets(off, n_seqs, rel)) return rc;
    std::vector<uint64_t> bin_off((size_t)n_seqs + 1, 0);
    for (uint32_t s = 0; s < n_seqs; ++s) bin_off[s + 1] = bin_off[s] + (rel[s + 1] - rel[s] + bin - 1) / bin;
    if (bin_off[n_seqs] != n_bins)
        return fail(HYPO_E_INVALID, "n_bins = %llu, the sequences have %llu bins of %u", (unsigned long long)n_bins, (unsigned long long)bin_off[n_seqs], bin);
    if (!n_bins) return HYPO_OK;                                       // (every sequence is empty)
    if (!bytes || !windows || !missing || !rated || !over || !under || !med_count) return fail(HYPO_E_INVALID, "NULL buffer");
    if (n_bins >= ((uint64_t)1 << 32)) return fail(HYPO_E_INVALID, "n_bins = %llu: at most 2^32 - 1 bins a call", (unsigned long long)n_bins);
    hipStream_t st = g_ctx.stream;
    Carver co, cr;
    co.take(rel.size() * 8);
    const size_t at_bin = co.take(bin_off.size() * 8);
    const size_t o_win = cr.take((size_t)n_bins * 4), o_mis = cr.take((size_t)n_bins * 4), o_rat = cr.take((size_t)n_bins * 4), o_ov = cr.take((size_t)n_bins * 4),
                 o_un = cr.take((size_t)n_bins * 4), o_med = cr.take((size_t)n_bins);
    KsDev d;
    if (const int rc = ks_arenas(ks, rel.back(), co.at, cr.at, d)) return rc;
    HIP_TRY(d.in.up(0, bytes + off[0], rel.back()));
    HIP_TRY(d.off.up(0, rel.data(), rel.size() * 8));
    HIP_TRY(d.off.up(at_bin, bin_off.data(), bin_off.size() * 8));
    const hypo::KsetDepthOut out{d.res.u32(o_win), d.res.u32(o_mis), d.res.u32(o_rat), d.res.u32(o_ov), d.res.u32(o_un), d.res.u8(o_med)};
    HIP_TRY(hypo::kset_depth_run(ks.view(), d.in.u8(0), d.off.u64(0), d.off.u64(at_bin), n_seqs, n_bins, bin, text, unit, out, st));
    HIP_TRY(d.res.down(windows, o_win, (size_t)n_bins * 4)); HIP_TRY(d.res.down(missing, o_mis, (size_t)n_bins * 4));
    HIP_TRY(d.res.down(rated, o_rat, (size_t)n_bins * 4)); HIP_TRY(d.res.down(over, o_ov, (size_t)n_bins * 4));
    HIP_TRY(d.res.down(under, o_un, (size_t)n_bins * 4)); HIP_TRY(d.res.down(med_count, o_med, (size_t)n_bins));
    HIP_TRY(hipStreamSynchronize(st));
    return HYPO_OK;
}

// ---- the set's records out and in (hypo --qv-save / --qv-load) ---------------------------------------------------------------------
// The cursor of an export sequence is the first slot the next call looks at: a call takes at most `cap` slots, so it never has more
// than `cap` records.  Arenas: ks.in holds the call's keys and, behind them, its count bytes; ks.off the tile sums and prefixes;
// ks.res the digest.
int hypo_gpu_kset_export(uint64_t* cursor, uint64_t* keys, uint8_t* counts, uint64_t cap, uint64_t* n_out, uint64_t* digest) {
    HYPO_KSET_ENTRY();
    if (!cursor || !keys || !n_out) return fail(HYPO_E_INVALID, "NULL buffer");
    if (!cap || cap >= ((uint64_t)1 << 32)) return fail(HYPO_E_INVALID, "cap = %llu out of range 1..2^32 - 1", (unsigned long long)cap);
    const uint64_t s0 = *cursor;
    if (s0 == HYPO_KSET_EXPORT_END) { *n_out = 0; return HYPO_OK; }  // (the sequence has ended: nothing more comes)
    if (s0 >= ks.slots) return fail(HYPO_E_INVALID, "cursor = %llu is no position in a table of %llu slots", (unsigned long long)s0, (unsigned long long)ks.slots);
    const uint64_t n_slots = ks.slots - s0 < cap ? ks.slots - s0 : cap;
    const uint32_t tiles = hypo::kset_export_tiles(n_slots);
    hipStream_t st = g_ctx.stream;
    HIP_TRY(ks.in.alloc((size_t)n_slots * 9));
    HIP_TRY(ks.off.alloc(((size_t)tiles * 2 + 1) * 8));
    HIP_TRY(ks.res.alloc(8));
    uint64_t* d_keys = (uint64_t*)ks.in.p;
    uint8_t* d_counts = (uint8_t*)ks.in.p + (size_t)n_slots * 8;
    uint64_t* d_sums = (uint64_t*)ks.off.p;
    uint64_t* d_pre = d_sums + tiles;
    uint64_t got[2] = {0, 0};                                           // the records of the call, their digest
    HIP_TRY(hipMemsetAsync(ks.res.p, 0, 8, st));
    HIP_TRY(hypo::kset_export_run(ks.table, ks.planes, s0, n_slots, d_sums, d_pre, n_slots, d_keys, counts ? d_counts : nullptr,
                                  (unsigned long long*)ks.res.p, st));
    // the number of records comes back first: only the used prefix of the two arrays is copied
    HIP_TRY(hipMemcpyAsync(&got[0], d_pre + tiles, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&got[1], ks.res.p, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (got[0] > n_slots) return fail(HYPO_E_HIP, "k-mer set: internal error: %llu records in %llu slots", (unsigned long long)got[0], (unsigned long long)n_slots);
    if (got[0]) {
        HIP_TRY(hipMemcpyAsync(keys, d_keys, (size_t)got[0] * 8, hipMemcpyDeviceToHost, st));
        if (counts) HIP_TRY(hipMemcpyAsync(counts, d_counts, (size_t)got[0], hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    *n_out = got[0];
    if (digest) *digest += got[1];
    *cursor = s0 + n_slots == ks.slots ? HYPO_KSET_EXPORT_END : s0 + n_slots;
    return HYPO_OK;
}

int hypo_gpu_kset_import(const uint64_t* keys, const uint8_t* counts, uint64_t n, uint64_t* digest) {
    HYPO_KSET_ENTRY();
    if (ks.marked) return fail(HYPO_E_INVALID, "the k-mer set is closed: a text has been marked (hypo_gpu_kset_mark)");
    if (n >= ((uint64_t)1 << 32)) return fail(HYPO_E_INVALID, "n = %llu records: a call takes fewer than 2^32", (unsigned long long)n);
    if (!n) return HYPO_OK;
    if (!keys) return fail(HYPO_E_INVALID, "NULL buffer");
    hipStream_t st = g_ctx.stream;
    HIP_TRY(ks.in.alloc((size_t)n * 9));
    HIP_TRY(ks.res.alloc(24));
    uint64_t* d_keys = (uint64_t*)ks.in.p;
    uint8_t* d_counts = counts ? (uint8_t*)ks.in.p + (size_t)n * 8 : nullptr;
    unsigned long long* d_bad = (unsigned long long*)ks.res.p;          // [0] a record was refused, [1] the least such index, [2] the digest
    const unsigned long long fresh[3] = {0, ~0ull, 0};
    unsigned long long bad[2] = {0, 0};
    HIP_TRY(h2d(d_keys, keys, (size_t)n * 8, st));
    if (counts) HIP_TRY(h2d(d_counts, counts, (size_t)n, st));
    HIP_TRY(hipMemcpyAsync(d_bad, fresh, 24, hipMemcpyHostToDevice, st));
    // every record is looked at on the device before the table is touched
    HIP_TRY(hypo::kset_import_check_run(d_keys, d_counts, n, ks.k, d_bad, st));
    HIP_TRY(hipMemcpyAsync(bad, d_bad, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (bad[0]) {
        const uint64_t i = bad[1], key = keys[i];
        if (key >> (2 * ks.k)) return fail(HYPO_E_INVALID, "record %llu: the key 0x%llx is not below 4^%u", (unsigned long long)i, (unsigned long long)key, ks.k);
        if (counts && !counts[i]) return fail(HYPO_E_INVALID, "record %llu: the count byte is 0", (unsigned long long)i);
        return fail(HYPO_E_INVALID, "record %llu: the key 0x%llx is not canonical: its reverse complement is smaller", (unsigned long long)i, (unsigned long long)key);
    }
    if (const int rc = ks_make_room(ks, n, "records", st)) return rc;
    unsigned long long ctr[2] = {0, 0}, sum = 0;
    const hipError_t kset_import =
        ks_counted(ks, ctr, st, [&](unsigned long long* d_ctr) { return hypo::kset_import_run(d_keys, d_counts, n, ks.table, ks.slots, d_ctr, ks.planes, d_bad + 2, st); });
    HIP_TRY(kset_import);
    HIP_TRY(hipMemcpyAsync(&sum, d_bad + 2, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    ks.count += ctr[0];
    if (ctr[1]) return fail(HYPO_E_HIP, "k-mer set: internal error: a table of %llu slots with %llu keys had no room", (unsigned long long)ks.slots, (unsigned long long)ks.count);
    if (digest) *digest += sum;
    return HYPO_OK;
}

int hypo_gpu_kset_end(void) {
    HYPO_LOCKED();
    HYPO_ON_DEVICE();
    Ctx::KSet& ks = g_ctx.ks;
    if (ks.k && getenv("HYPO_KSET_STATS"))
        fprintf(stderr, "[kset] k %u, %llu keys, %llu slots (peak %llu), %u growths in %.6f s\n", ks.k, (unsigned long long)ks.count,
                (unsigned long long)ks.slots, (unsigned long long)ks.peak_slots, ks.growths, ks.grow_s);
    if (ks.table) HIP_TRY(hipFree(ks.table));
    if (ks.planes) HIP_TRY(hipFree(ks.planes));
    for (DevBuf* d : {&ks.in, &ks.off, &ks.res, &ks.ctr}) d->release();
    ks = Ctx::KSet();
    return HYPO_OK;
}

// ---- edit scripts of the replacement units (edit_kernel.hip; hypo --vcf) ---------------------------------------------------------
// Runs the long or the wide list in chunks of at most chunk_bytes of move storage (option "edit_chunk_mb"; a pair that needs more
// runs alone).  need(e) = (moves bytes, values bytes).  launches: one more per chunk.
}  // extern "C"
template <class Need, class Launch>
static int edit_run_list(const uint4* dlist, const std::vector<uint4>& list, uint64_t chunk_bytes, uint64_t& launches, Need need, Launch launch) {
    Ctx::EditBufs& ed = g_ctx.ed;
    hipStream_t st = g_ctx.stream;
    std::vector<uint64_t> moff, voff;
    for (size_t e0 = 0; e0 < list.size();) {
        moff.clear(); voff.clear();
        uint64_t mb = 0, vb = 0;
        size_t e1 = e0;
        for (; e1 < list.size(); ++e1) {
            uint64_t m, v;
            need(list[e1], m, v);
            if (e1 > e0 && mb + m > chunk_bytes) break;
            // moves is addressed in bytes, vals in its int32 elements (edit_wide_run: `vals + vals_off[e]`)
            moff.push_back(mb); voff.push_back(vb / 4);
            mb += (m + 15) & ~15ull; vb += (v + 15) & ~15ull;
        }
        HIP_TRY(ed.moves.alloc(mb));
        HIP_TRY(ed.vals.alloc(vb));
        HIP_TRY(ed.moves_off.alloc(moff.size() * 8));
        HIP_TRY(ed.vals_off.alloc(voff.size() * 8));
        HIP_TRY(hipMemcpyAsync(ed.moves_off.p, moff.data(), moff.size() * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(ed.vals_off.p, voff.data(), voff.size() * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(launch(dlist + e0, (uint32_t)(e1 - e0)));
        HIP_TRY(hipStreamSynchronize(st));                    // (the offsets' host vectors are refilled for the next chunk)
        ++launches;
        e0 = e1;
    }
    return HYPO_OK;
}
extern "C" {

int hypo_gpu_edit_scripts(const HypoEditBatch* in, uint32_t* dist, uint64_t* run_off, uint32_t* runs, uint64_t runs_cap) {
    HYPO_ENTRY();
    if (!in || !run_off || (in->n_pairs && (!dist || !in->a_off || !in->b_off))) return fail(HYPO_E_INVALID, "NULL buffer");
    const uint32_t np = in->n_pairs;
    run_off[0] = 0;
    if (!np) return HYPO_OK;
    // offsets rebased to 0 and checked: monotone, every side below 2^30 bytes
    std::vector<uint64_t> aoff((size_t)np + 1), boff((size_t)np + 1);
    for (uint32_t p = 0; p <= np; ++p) {
        aoff[p] = in->a_off[p] - in->a_off[0]; boff[p] = in->b_off[p] - in->b_off[0];
        if (p && (in->a_off[p] < in->a_off[p - 1] || in->b_off[p] < in->b_off[p - 1] || aoff[p] - aoff[p - 1] >= (1u << 30) || boff[p] - boff[p - 1] >= (1u << 30)))
            return fail(HYPO_E_INVALID, "pair %u: offsets not monotone or a side of 2^30 bytes or more", p - 1);
    }
    if ((aoff[np] && !in->a) || (boff[np] && !in->b)) return fail(HYPO_E_INVALID, "NULL bytes");
    Ctx::EditBufs& ed = g_ctx.ed;
    Ctx::EditKept& kept = ed.kept;
    hipStream_t st = g_ctx.stream;
    // the retry of a call that answered HYPO_E_WORKSPACE: the same batch (pointers and offsets) copies the kept results out
    const bool reuse = kept.valid && kept.a == in->a && kept.b == in->b && kept.a0 == in->a_off[0] && kept.b0 == in->b_off[0] &&
                       kept.aoff == aoff && kept.boff == boff;
    kept.valid = false;
    if (!reuse) {
        HIP_TRY(ed.a.alloc(aoff[np])); HIP_TRY(ed.b.alloc(boff[np]));
        HIP_TRY(ed.a_off.alloc(((size_t)np + 1) * 8)); HIP_TRY(ed.b_off.alloc(((size_t)np + 1) * 8));
        HIP_TRY(ed.res.alloc((size_t)np * 12)); HIP_TRY(ed.lists.alloc((size_t)np * 48)); HIP_TRY(ed.ctr.alloc(32));
        if (aoff[np]) HIP_TRY(h2d(ed.a.p, in->a + in->a_off[0], aoff[np], st));
        if (boff[np]) HIP_TRY(h2d(ed.b.p, in->b + in->b_off[0], boff[np], st));
        HIP_TRY(h2d(ed.a_off.p, aoff.data(), aoff.size() * 8, st));
        HIP_TRY(h2d(ed.b_off.p, boff.data(), boff.size() * 8, st));
        hypo::EditIO io{};
        io.a = (const char*)ed.a.p; io.b = (const char*)ed.b.p; io.a_off = (const uint64_t*)ed.a_off.p; io.b_off = (const uint64_t*)ed.b_off.p;
        io.n_pairs = np;
        io.dist = (uint32_t*)ed.res.p; io.rstart = io.dist + np; io.rcount = io.rstart + np;
        io.counters = (unsigned long long*)ed.ctr.p;
        io.long_list = (uint4*)ed.lists.p; io.wide_list = io.long_list + np; io.wide_list2 = io.wide_list + np;
        unsigned long long ctr[4] = {0, 0, 0, 0};
        // the pool starts at 4 runs per pair (the polishing runs measured 2.2 - 2.6) or what the context has; a call that overflows it
        // (counted, never written past) runs again with the size it reported, and the grown pool stays for the calls after it
        HIP_TRY(ed.pool.alloc(std::max<size_t>(ed.pool.cap, ((size_t)np * 4 + 1024) * 4)));
        const uint64_t chunk_bytes = g_edit_chunk_bytes.load();
        uint64_t n_long = 0, n_wide = 0, n_second = 0, long_launches = 0, wide_launches = 0, passes = 0;
        for (int attempt = 0;; ++attempt) {
            n_long = n_wide = n_second = long_launches = wide_launches = 0; ++passes;
            io.pool = (uint32_t*)ed.pool.p; io.pool_cap = ed.pool.cap / 4;
            HIP_TRY(hipMemsetAsync(ed.ctr.p, 0, 32, st));
            HIP_TRY(hypo::edit_fast_run(io, g_ctx.num_cus, st));
            HIP_TRY(hipMemcpyAsync(ctr, ed.ctr.p, 32, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            if (ctr[1]) {                                        // pairs whose move codes do not fit in LDS
                std::vector<uint4> list((size_t)ctr[1]);
                HIP_TRY(hipMemcpyAsync(list.data(), io.long_list, list.size() * 16, hipMemcpyDeviceToHost, st));
                HIP_TRY(hipStreamSynchronize(st));
                n_long = list.size();
                const int rc = edit_run_list(io.long_list, list, chunk_bytes, long_launches, [&](const uint4& e, uint64_t& mb, uint64_t& vb) {
                    mb = 16 * (aoff[e.x + 1] - aoff[e.x] + boff[e.x + 1] - boff[e.x] - 2 * e.y + 2); vb = 0;
                }, [&](const uint4* dl, uint32_t n) { return hypo::edit_long_run(io, dl, n, (uint8_t*)ed.moves.p, (const uint64_t*)ed.moves_off.p, st); });
                if (rc != HYPO_OK) return rc;
                HIP_TRY(hipMemcpyAsync(ctr, ed.ctr.p, 32, hipMemcpyDeviceToHost, st));
                HIP_TRY(hipStreamSynchronize(st));
            }
            // pairs the 128-diagonal band cannot decide (with their d_b), or cannot hold (probes); then the probes that were not exact
            for (int w = 0; w < 2; ++w) {
                if (w) { HIP_TRY(hipMemcpyAsync(ctr, ed.ctr.p, 32, hipMemcpyDeviceToHost, st)); HIP_TRY(hipStreamSynchronize(st)); }
                uint4* dlist = w ? io.wide_list2 : io.wide_list;
                if (!ctr[2 + w]) continue;
                std::vector<uint4> list((size_t)ctr[2 + w]);
                HIP_TRY(hipMemcpyAsync(list.data(), dlist, list.size() * 16, hipMemcpyDeviceToHost, st));
                HIP_TRY(hipStreamSynchronize(st));
                (w ? n_second : n_wide) = list.size();
                const int rc = edit_run_list(dlist, list, chunk_bytes, wide_launches, [&](const uint4& e, uint64_t& mb, uint64_t& vb) {
                    const uint32_t n = (uint32_t)(aoff[e.x + 1] - aoff[e.x]) - e.y, m = (uint32_t)(boff[e.x + 1] - boff[e.x]) - e.y;
                    int64_t lo, hi;
                    hypo::edit_wide_band(n, m, e.z, lo, hi);
                    mb = 16 * hypo::edit_wide_groups(lo, hi) * ((uint64_t)n + m + 2);
                    vb = (uint64_t)(hi - lo + 1) > hypo::EDIT_WIDE_LDS_DIAGS ? 4 * (uint64_t)(hi - lo + 1) : 0;
                }, [&](const uint4* dl, uint32_t n) {
                    return hypo::edit_wide_run(io, dl, n, (uint8_t*)ed.moves.p, (const uint64_t*)ed.moves_off.p, (int32_t*)ed.vals.p, (const uint64_t*)ed.vals_off.p, st);
                });
                if (rc != HYPO_OK) return rc;
            }
            HIP_TRY(hipMemcpyAsync(ctr, ed.ctr.p, 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            if (ctr[0] >= (1ull << 32)) return fail(HYPO_E_CAPACITY, "%llu runs in one call: split the batch", ctr[0]);
            if (ctr[0] <= io.pool_cap) break;
            if (attempt) return fail(HYPO_E_HIP, "edit run pool overflowed twice (%llu runs, capacity %llu)", ctr[0], (unsigned long long)io.pool_cap);
            HIP_TRY(ed.pool.alloc((size_t)ctr[0] * 4));
        }
        kept.res.resize((size_t)np * 3);
        HIP_TRY(d2h(kept.res.data(), ed.res.p, kept.res.size() * 4, st));
        HIP_TRY(hipStreamSynchronize(st));
        kept.a = in->a; kept.b = in->b; kept.a0 = in->a_off[0]; kept.b0 = in->b_off[0]; kept.n_runs = ctr[0];
        kept.aoff.swap(aoff); kept.boff.swap(boff);
        const uint64_t counts[8] = {np, n_long, n_wide, n_second, ctr[0], passes, long_launches, wide_launches};
        memcpy(ed.last_counts, counts, sizeof counts);
    }
    const uint32_t *rstart = kept.res.data() + np, *rcount = rstart + np;
    for (uint32_t p = 0; p < np; ++p) run_off[p + 1] = run_off[p] + rcount[p];
    memcpy(dist, kept.res.data(), (size_t)np * 4);
    if (runs_cap < run_off[np]) {
        kept.valid = true;
        return fail(HYPO_E_WORKSPACE, "runs_cap %llu < %llu runs", (unsigned long long)runs_cap, (unsigned long long)run_off[np]);
    }
    if (run_off[np] && !runs) return fail(HYPO_E_INVALID, "NULL runs");
    std::vector<uint32_t> pool((size_t)kept.n_runs);
    if (kept.n_runs) HIP_TRY(d2h(pool.data(), ed.pool.p, pool.size() * 4, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (uint32_t p = 0; p < np; ++p) memcpy(runs + run_off[p], pool.data() + rstart[p], (size_t)rcount[p] * 4);
    return HYPO_OK;
}

int hypo_gpu_edit_last_counts(uint64_t out[8]) {
    HYPO_LOCKED();
    if (!out) return fail(HYPO_E_INVALID, "NULL");
    if (!g_ctx.ready) return fail(HYPO_E_NOTINIT, "hypo_gpu_init was not called");
    memcpy(out, g_ctx.ed.last_counts, sizeof g_ctx.ed.last_counts);
    return HYPO_OK;
}

int hypo_gpu_host_alloc(size_t bytes, void** out) {
    if (!out) return fail(HYPO_E_INVALID, "NULL");
    *out = nullptr;
    HYPO_ON_DEVICE();
    if (!g_ctx.ready) return fail(HYPO_E_NOTINIT, "hypo_gpu_init was not called");
    HIP_TRY(hipHostMalloc(out, bytes ? bytes : 16, hipHostMallocDefault));
    return HYPO_OK;
}
int hypo_gpu_host_free(void* p) {
    if (!p) return HYPO_OK;
    HIP_TRY(hipHostFree(p));
    return HYPO_OK;
}
int hypo_gpu_host_register(void* p, size_t bytes) {
    if (!p || !bytes) return fail(HYPO_E_INVALID, "NULL / empty range");
    HYPO_ON_DEVICE();
    if (!g_ctx.ready) return fail(HYPO_E_NOTINIT, "hypo_gpu_init was not called");
    HIP_TRY(hipHostRegister(p, bytes, hipHostRegisterDefault));
    return HYPO_OK;
}
int hypo_gpu_host_unregister(void* p) {
    if (!p) return HYPO_OK;
    HIP_TRY(hipHostUnregister(p));
    return HYPO_OK;
}

// ---- support votes on the device (kernels in support_kernel.hip) -----------------------------------------

int hypo_gpu_reads_upload(const HypoArmsReads* A, const uint32_t* read_contig, uint64_t total_len) {
    HYPO_ENTRY();
    auto& rr = g_ctx.rr;
    rr.ready = false;
    if (!A || !read_contig) return fail(HYPO_E_INVALID, "NULL argument");
    const uint32_t na = A->n_alignments;
    if (na && (!A->rb || !A->re || !A->qae || !A->seq_off || !A->reads2 || !A->cigar_off || !A->cigar)) return fail(HYPO_E_INVALID, "NULL buffer in reads");
    uint32_t max_span = 0; uint64_t sum_span = 0;
    rr.ctg_min_rb.clear(); rr.ctg_max_re.clear();
    {   // every record is checked before anything is sent (10 M records per 50 Mbp batch: 40 ms on one thread, so eight share them)
        struct Part { uint32_t bad = 0xffffffffu; ReadFault why = READ_OK; uint32_t max_span = 0; uint64_t sum_span = 0; std::vector<uint32_t> lo, hi; };
        const int P = na >= (1u << 18) ? 8 : 1;
        std::vector<Part> part((size_t)P);
        auto run = [&](int t) {
            Part& pt = part[(size_t)t];
            const uint32_t a0 = (uint32_t)((uint64_t)na * (uint64_t)t / (uint64_t)P), a1 = (uint32_t)((uint64_t)na * ((uint64_t)t + 1) / (uint64_t)P);
            for (uint32_t a = a0; a < a1; ++a) {
                if (const ReadFault why = read_fault(*A, a, total_len, read_contig)) { pt.bad = a; pt.why = why; return; }
                const uint32_t span = A->re[a] - A->rb[a];
                pt.max_span = span > pt.max_span ? span : pt.max_span;
                pt.sum_span += span;
                const uint32_t rc = read_contig[a];
                if (rc >= pt.lo.size()) { pt.lo.resize((size_t)rc + 1, 0xffffffffu); pt.hi.resize((size_t)rc + 1, 0u); }
                if (A->rb[a] < pt.lo[rc]) pt.lo[rc] = A->rb[a];
                if (A->re[a] > pt.hi[rc]) pt.hi[rc] = A->re[a];
            }
        };
        std::vector<std::thread> th;
        for (int t = 1; t < P; ++t) th.emplace_back(run, t);
        run(0);
        for (auto& x : th) x.join();
        for (const Part& pt : part) {
            if (pt.bad != 0xffffffffu) return read_fail(pt.why, *A, pt.bad, total_len, read_contig);      // (parts are in record order: this is the first bad record)
            max_span = pt.max_span > max_span ? pt.max_span : max_span;
            sum_span += pt.sum_span;
            if (pt.lo.size() > rr.ctg_min_rb.size()) { rr.ctg_min_rb.resize(pt.lo.size(), 0xffffffffu); rr.ctg_max_re.resize(pt.lo.size(), 0u); }
            for (size_t c = 0; c < pt.lo.size(); ++c) {
                if (pt.lo[c] < rr.ctg_min_rb[c]) rr.ctg_min_rb[c] = pt.lo[c];
                if (pt.hi[c] > rr.ctg_max_re[c]) rr.ctg_max_re[c] = pt.hi[c];
            }
        }
    }
    rr.total_len = total_len;
    Carver c;
    const size_t o_ctg = c.take((size_t)na * 4);
    hipStream_t st = g_ctx.stream;
    if (const int rc = reads_to_device(c, rr.data, *A, st, rr.dev)) return rc;
    const DevAt d{(char*)rr.data.p, st};
    HIP_TRY(d.up(o_ctg, read_contig, (size_t)na * 4));
    HIP_TRY(hipStreamSynchronize(st));                          // the caller may release its arrays
    rr.n = na; rr.reads2_bytes = A->reads2_bytes; rr.max_span = max_span; rr.sum_span = sum_span; rr.read_contig = d.u32(o_ctg);
    rr.ready = true;
    return HYPO_OK;
}

static hypo::SupportReads support_reads_of(const Ctx& c) {
    hypo::SupportReads R;
    const Ctx::DevReads& d = c.rr.dev;
    R.n_alignments = c.rr.n; R.rb = d.rb; R.re = d.re; R.qae = d.qae; R.seq_off = d.seq_off; R.reads2 = d.reads2; R.read_contig = c.rr.read_contig;
    R.mean_span = c.rr.n ? (uint32_t)(c.rr.sum_span / c.rr.n) : 0u;
    return R;
}

int hypo_gpu_support_kmers(uint32_t k, uint64_t n_solid, const uint32_t* spos, const uint64_t* kids, uint32_t* coverage, uint32_t* support) {
    HYPO_VOTE_ENTRY();
    if (const int rc = check_k(k)) return rc;
    if (n_solid >= 0xfffffff0ull) return fail(HYPO_E_CAPACITY, "%llu solid k-mers exceed the 32-bit counters of the boundary", (unsigned long long)n_solid);
    if (n_solid && (!spos || !kids || !coverage || !support)) return fail(HYPO_E_INVALID, "NULL buffer");
    if (!n_solid) return HYPO_OK;
    for (uint64_t i = 1; i < n_solid; ++i) if (spos[i - 1] >= spos[i]) return fail(HYPO_E_INVALID, "solid positions are not increasing (entry %llu)", (unsigned long long)i);
    Carver c;
    const size_t o_sp = c.take(n_solid * 4), o_kd = c.take(n_solid * 8), o_cov = c.take(n_solid * 4), o_sup = c.take(n_solid * 4);
    HIP_TRY(g_ctx.rr.work.alloc(c.at));
    const DevAt d{(char*)g_ctx.rr.work.p, g_ctx.stream};
    HIP_TRY(h2d(d.u32(o_sp), spos, n_solid * 4, d.st));
    HIP_TRY(h2d(d.u64(o_kd), kids, n_solid * 8, d.st));
    return vote_run(d, o_cov, o_sup, c.at, n_solid, coverage, support, [&](uint32_t* cov, uint32_t* sup) -> int {
        HIP_TRY(hypo::support_kmers(support_reads_of(g_ctx), k, (uint32_t)n_solid, d.u32(o_sp), d.u64(o_kd), cov, sup, d.st));
        return HYPO_OK;
    });
}

int hypo_gpu_support_kmers_kept(uint32_t k, uint32_t n_contigs, const uint32_t* handles, const uint32_t* contig_base,
                                uint32_t* coverage, uint32_t* support, uint64_t* n_solid_total) {
    HYPO_VOTE_ENTRY();
    if (const int rc = check_k(k)) return rc;
    if (n_contigs && (!handles || !contig_base)) return fail(HYPO_E_INVALID, "NULL argument");
    uint64_t ns = 0;
    for (uint32_t c = 0; c < n_contigs; ++c) {
        if (handles[c] >= g_ctx.kept.size() || !g_ctx.kept[handles[c]].used) return fail(HYPO_E_INVALID, "contig %u: handle %u holds no scan on this context", c, handles[c]);
        const Ctx::KeptScan& ks = g_ctx.kept[handles[c]];
        if (ks.k != k) return fail(HYPO_E_INVALID, "contig %u was scanned with k = %u", c, ks.k);
        if ((uint64_t)contig_base[c] + ks.n_bases > g_ctx.rr.total_len) return fail(HYPO_E_INVALID, "contig %u ends behind the %llu bases of the resident reads", c, (unsigned long long)g_ctx.rr.total_len);
        if (c && (uint64_t)contig_base[c] < (uint64_t)contig_base[c - 1] + g_ctx.kept[handles[c - 1]].n_bases) return fail(HYPO_E_INVALID, "contig %u overlaps the one before it", c);
        ns += ks.n;
    }
    if (n_solid_total) *n_solid_total = ns;
    if (ns >= 0xfffffff0ull) return fail(HYPO_E_CAPACITY, "%llu solid k-mers exceed the 32-bit counters of the boundary", (unsigned long long)ns);
    if (!ns) return HYPO_OK;
    if (!coverage || !support) return fail(HYPO_E_INVALID, "NULL buffer");
    const bool narrow = k <= 16;
    const size_t kid_bytes = narrow ? 4 : 8;
    Carver c;
    const size_t o_sp = c.take(ns * 4), o_kd = c.take(ns * kid_bytes), o_cov = c.take(ns * 4), o_sup = c.take(ns * 4);
    HIP_TRY(g_ctx.rr.work.alloc(c.at));
    const DevAt d{(char*)g_ctx.rr.work.p, g_ctx.stream};
    uint64_t at = 0;
    for (uint32_t ci = 0; ci < n_contigs; ++ci) {
        const Ctx::KeptScan& ks = g_ctx.kept[handles[ci]];
        if (!ks.n) continue;
        HIP_TRY(hypo::add_base(ks.spos, d.u32(o_sp) + at, ks.n, contig_base[ci], d.st));
        HIP_TRY(hipMemcpyAsync(d.u8(o_kd + at * kid_bytes), ks.kids, ks.n * kid_bytes, hipMemcpyDeviceToDevice, d.st));
        at += ks.n;
    }
    return vote_run(d, o_cov, o_sup, c.at, ns, coverage, support, [&](uint32_t* cov, uint32_t* sup) -> int {
        if (narrow) HIP_TRY(hypo::support_kmers32(support_reads_of(g_ctx), k, (uint32_t)ns, d.u32(o_sp), d.u32(o_kd), cov, sup, d.st));
        else HIP_TRY(hypo::support_kmers(support_reads_of(g_ctx), k, (uint32_t)ns, d.u32(o_sp), d.u64(o_kd), cov, sup, d.st));
        return HYPO_OK;
    });
}

int hypo_gpu_support_minimizers(const HypoMegaWindows* W, uint32_t* coverage, uint32_t* support) {
    HYPO_VOTE_ENTRY();
    if (!W || !W->n_contigs || !W->contig_base || !W->reg_base || !W->win_even || !W->info_base || !W->start || !W->mw_off) return fail(HYPO_E_INVALID, "NULL argument");
    const uint32_t nc = W->n_contigs;
    const uint64_t n_start = W->reg_base[nc], n_ent = W->mw_off[W->n_info];
    if (n_ent && (!W->rel_pos || !W->minimisers || !coverage || !support)) return fail(HYPO_E_INVALID, "NULL buffer");
    if (!n_ent) return HYPO_OK;
    for (uint32_t c = 0; c < nc; ++c) {
        if (W->reg_base[c] > W->reg_base[c + 1]) return fail(HYPO_E_INVALID, "contig %u: reg_base decreases", c);
        for (uint64_t i = W->reg_base[c] + 1; i < W->reg_base[c + 1]; ++i) if (W->start[i - 1] >= W->start[i]) return fail(HYPO_E_INVALID, "contig %u: region starts are not increasing", c);
    }
    for (uint32_t x = 0; x < W->n_info; ++x) if (W->mw_off[x] > W->mw_off[x + 1]) return fail(HYPO_E_INVALID, "mw_off decreases at %u", x);
    // the tables against the resident reads (another caller than DeviceArms may pass tables of other contigs): every read's contig
    // exists, its span lies inside that contig, and the MWMinimiserInfo entries its mega-windows index exist (a read that ends in
    // the last region looks at entry info_base + (borders - 1) / 2, one past the contig's last: mw_off is padded by one on the device)
    {
        const auto& rr = g_ctx.rr;
        if (rr.ctg_min_rb.size() > nc) return fail(HYPO_E_INVALID, "the resident reads name contig %zu, the tables hold %u contigs", rr.ctg_min_rb.size() - 1, nc);
        for (uint32_t c = 0; c < nc; ++c) {
            const uint32_t nb = W->reg_base[c + 1] - W->reg_base[c];
            const bool has_reads = c < rr.ctg_min_rb.size() && rr.ctg_max_re[c] > 0;
            if (!has_reads) continue;
            if (nb < 2) return fail(HYPO_E_INVALID, "contig %u has reads but fewer than two region borders", c);
            const uint64_t len = W->start[W->reg_base[c + 1] - 1];
            if (rr.ctg_min_rb[c] < W->contig_base[c] || (uint64_t)rr.ctg_max_re[c] > (uint64_t)W->contig_base[c] + len)
                return fail(HYPO_E_INVALID, "contig %u: its resident reads span [%u, %u), the tables place it at [%u, %llu)", c, rr.ctg_min_rb[c], rr.ctg_max_re[c],
                            W->contig_base[c], (unsigned long long)((uint64_t)W->contig_base[c] + len));
            if ((uint64_t)W->info_base[c] + (nb - 1) / 2 > (uint64_t)W->n_info)
                return fail(HYPO_E_INVALID, "contig %u: %u region borders need MWMinimiserInfo entries up to %llu, the tables hold %u", c, nb,
                            (unsigned long long)((uint64_t)W->info_base[c] + (nb - 1) / 2), W->n_info);
        }
    }
    Carver c;
    const size_t o_cb = c.take((size_t)nc * 4), o_rbase = c.take((size_t)(nc + 1) * 4), o_even = c.take(nc), o_ib = c.take((size_t)nc * 4), o_start = c.take(n_start * 4),
                 o_off = c.take((size_t)(W->n_info + 2) * 4), o_rel = c.take(n_ent * 4), o_min = c.take(n_ent * 4), o_cov = c.take(n_ent * 4), o_sup = c.take(n_ent * 4);
    HIP_TRY(g_ctx.rr.work.alloc(c.at));
    const DevAt d{(char*)g_ctx.rr.work.p, g_ctx.stream};
    HIP_TRY(d.up(o_cb, W->contig_base, (size_t)nc * 4)); HIP_TRY(d.up(o_rbase, W->reg_base, (size_t)(nc + 1) * 4)); HIP_TRY(d.up(o_even, W->win_even, nc));
    HIP_TRY(d.up(o_ib, W->info_base, (size_t)nc * 4)); HIP_TRY(d.up(o_start, W->start, n_start * 4)); HIP_TRY(d.up(o_off, W->mw_off, (size_t)(W->n_info + 1) * 4));
    HIP_TRY(d.up(o_rel, W->rel_pos, n_ent * 4)); HIP_TRY(d.up(o_min, W->minimisers, n_ent * 4));
    HIP_TRY(d.up(o_off + (size_t)(W->n_info + 1) * 4, W->mw_off + W->n_info, 4));          // the pad entry: an empty range behind the last info
    hypo::MegaWindows M;
    M.contig_base = d.u32(o_cb); M.reg_base = d.u32(o_rbase); M.win_even = d.u8(o_even); M.info_base = d.u32(o_ib);
    M.start = d.u32(o_start); M.mw_off = d.u32(o_off); M.rel_pos = d.u32(o_rel); M.minimisers = d.u32(o_min);
    return vote_run(d, o_cov, o_sup, c.at, n_ent, coverage, support, [&](uint32_t* cov, uint32_t* sup) -> int {
        HIP_TRY(hypo::support_minimizers(support_reads_of(g_ctx), M, nc, W->n_info, cov, sup, d.st));
        return HYPO_OK;
    });
}

// ---- arm selection on the device (kernels in arms_kernel.hip) ------------------------------------------

// which = 0: short reads -> SHORT windows; 1: long reads over the pseudo regions of Contig::prepare_long_windows -> LONG windows
static int arms_build_impl(int which, const HypoArmsRegions* R, const HypoArmsReads* A, uint8_t* region_valid, HypoArmsSummary* sum) {
    HYPO_ENTRY();
    auto& AS = g_ctx.arms[which];
    const bool long_mode = which == 1;
    if (!R || !region_valid || !sum) return fail(HYPO_E_INVALID, "NULL argument");
    // reads == NULL: the reads hypo_gpu_reads_upload left on the device (already checked there)
    const bool resident = A == nullptr;
    if (resident && (long_mode || !g_ctx.rr.ready)) return fail(HYPO_E_INVALID, "reads == NULL but no resident reads (hypo_gpu_reads_upload)");
    HypoArmsReads Ares{};
    if (resident) { Ares.n_alignments = g_ctx.rr.n; Ares.reads2_bytes = g_ctx.rr.reads2_bytes; A = &Ares; }
    if (!R->n_regions || !R->start || !R->type || (!long_mode && !R->info) || !R->contig4 || (R->n_anchor_kmers && !R->anchor_kmers)) return fail(HYPO_E_INVALID, "NULL buffer in regions");
    if (!resident && A->n_alignments && (!A->rb || !A->re || !A->qae || !A->seq_off || !A->reads2 || !A->cigar_off || !A->cigar)) return fail(HYPO_E_INVALID, "NULL buffer in reads");
    if (const int rc = check_k(R->k)) return rc;
    AS.ready = false;
    const uint32_t nr = R->n_regions, na = A->n_alignments;
    const uint64_t total_len = R->start[nr];
    uint32_t max_span = 0;
    uint64_t sum_span = 0;
    for (uint32_t i = 0; i < nr; ++i) if (R->start[i] >= R->start[i + 1]) return fail(HYPO_E_INVALID, "region %u is empty or the starts are not increasing", i);
    if (resident) {
        if (total_len != g_ctx.rr.total_len)
            return fail(HYPO_E_INVALID, "the regions cover %llu bases, the resident reads were checked against %llu (hypo_gpu_reads_upload)", (unsigned long long)total_len, (unsigned long long)g_ctx.rr.total_len);
        max_span = g_ctx.rr.max_span; sum_span = g_ctx.rr.sum_span;
    }
    for (uint32_t a = 0; a < (resident ? 0u : na); ++a) {
        if (const ReadFault why = read_fault(*A, a, total_len, nullptr)) return read_fail(why, *A, a, total_len, nullptr);
        const uint32_t span = A->re[a] - A->rb[a];
        max_span = span > max_span ? span : max_span;
        sum_span += span;
    }
    // arms_window_kernel looks, per window, at every alignment that starts within max_span bases before it: one record with a
    // huge reference span (a 100 kb D / N operation) would make every window walk a 100 kb neighbourhood.  Such input takes the
    // host loops (the caller falls back on any error of this call).
    if (na && max_span > 16384u && (uint64_t)max_span * na > 64ull * sum_span)
        return fail(HYPO_E_CAPACITY, "an alignment spans %u reference bases, more than 64 x the mean span (%llu): arm selection stays on the host",
                    max_span, (unsigned long long)(sum_span / na));
    hipStream_t st = g_ctx.stream;
    DevBuf &dIn = AS.arena[0], &dWork = AS.arena[1], &dBatch = AS.arena[2];
    // inputs: the regions, then the reads unless they are resident
    Carver ci;
    const size_t o_start = ci.take((size_t)(nr + 1) * 4), o_type = ci.take(nr + 1), o_info = ci.take((size_t)(nr + 1) * 4),
                 o_anchor = ci.take(R->n_anchor_kmers * 8), o_contig = ci.take((total_len + 1) / 2);
    Ctx::DevReads dr = g_ctx.rr.dev;
    if (resident) HIP_TRY(dIn.alloc(ci.at));
    else if (const int rc = reads_to_device(ci, dIn, *A, st, dr)) return rc;
    const DevAt in{(char*)dIn.p, st};
    HIP_TRY(in.up(o_start, R->start, (size_t)(nr + 1) * 4)); HIP_TRY(in.up(o_type, R->type, (size_t)nr + 1)); if (R->info) HIP_TRY(in.up(o_info, R->info, (size_t)(nr + 1) * 4));
    HIP_TRY(in.up(o_anchor, R->anchor_kmers, R->n_anchor_kmers * 8)); HIP_TRY(in.up(o_contig, R->contig4, (total_len + 1) / 2));
    hypo::ArmsIn I;
    I.n_regions = nr; I.reg_start = in.u32(o_start); I.reg_type = in.u8(o_type); I.reg_info = in.u32(o_info); I.anchor_kmers = in.u64(o_anchor); I.k = R->k; I.contig4 = in.u8(o_contig);
    I.n_alignments = na; I.rb = dr.rb; I.re = dr.re; I.qae = dr.qae; I.seq_off = dr.seq_off; I.reads2 = dr.reads2; I.cigar_off = dr.cigar_off; I.cigar = dr.cigar;
    I.file_rank = dr.file_rank; I.max_span = max_span; I.long_mode = long_mode ? 1u : 0u;
    // work arrays that do not depend on the number of touched regions
    Carver cw;
    const size_t scan_n = nr > na ? nr : na;
    const size_t w_bind = cw.take((size_t)na * 4), w_nt = cw.take((size_t)na * 4), w_toff = cw.take((size_t)na * 8), w_bsum = cw.take(hypo::scan32_scratch_bytes(scan_n)),
                 w_tot = cw.take(64), w_flags = cw.take((size_t)nr * 4), w_valid = cw.take((size_t)nr * 4), w_counts = cw.take((size_t)nr * 16),
                 w_arms = cw.take((size_t)nr * 4), w_bytes = cw.take((size_t)nr * 4), w_bint = cw.take((size_t)nr * 4), w_bpre = cw.take((size_t)nr * 4),
                 w_dbytes = cw.take((size_t)nr * 4), w_slot = cw.take((size_t)nr * 4), w_winoff = cw.take((size_t)nr * 8), w_armoff = cw.take((size_t)nr * 8),
                 w_byteoff = cw.take((size_t)nr * 8), w_droff = cw.take((size_t)nr * 8), w_slotoff = cw.take((size_t)nr * 8), w_widx = cw.take((size_t)nr * 4),
                 w_minlen = cw.take(long_mode ? (size_t)nr * 4 : 0), w_minoff = cw.take(long_mode ? (size_t)nr * 8 : 0), w_mincnt = cw.take(long_mode ? (size_t)nr * 4 : 0);
    const size_t fixed_work = cw.at;
    // the candidate arrays follow: a read of span s touches at most s / (shortest region) + 2 regions; sized after phase 1
    HIP_TRY(dWork.alloc(fixed_work));
    const DevAt wk{(char*)dWork.p, st};
    uint64_t* tot = wk.u64(w_tot);             // [0] touched regions, [1] windows, [2] arms, [3] arm bytes, [4] draft bytes, [5] slot bytes, [6] bad records
    HIP_TRY(hipMemsetAsync(tot, 0, 64, st));
    HIP_TRY(hypo::arms_phase1(I, wk.u32(w_bind), wk.u32(w_nt), (uint32_t*)(tot + 6), st));
    HIP_TRY(hypo::scan32(wk.u32(w_nt), na, wk.u64(w_toff), wk.u64(w_bsum), tot + 0, st));
    hypo::ArmsOut O{};
    if (long_mode) {      // slots for the minimizers of every LONG window's draft (Filter::initialise): one per base at most
        O.reg_min_len = wk.u32(w_minlen); O.reg_min_off = wk.u64(w_minoff); O.reg_min_cnt = wk.u32(w_mincnt);
        HIP_TRY(hypo::arms_long_minlen(I, O, st));
        HIP_TRY(hypo::scan32(O.reg_min_len, nr, wk.u64(w_minoff), wk.u64(w_bsum), tot + 7, st));
    }
    uint64_t h_tot[8] = {0};
    HIP_TRY(hipMemcpyAsync(h_tot, tot, 64, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (h_tot[6]) return fail(HYPO_E_INVALID, "%llu alignment record(s) whose CIGAR disagrees with their span / aligned length", (unsigned long long)h_tot[6]);
    const uint64_t n_touch = h_tot[0];
    // candidates (in a buffer of their own: growing dWork would move the arrays phase 1 filled)
    DevBuf& dCand = AS.arena[3];
    Carver cc;
    const size_t c_bp = cc.take(n_touch * 4), c_cand = cc.take(n_touch * 8), c_dmin = cc.take(long_mode ? h_tot[7] * 4 + 16 : 0);
    HIP_TRY(dCand.alloc(cc.at));
    const DevAt cd{(char*)dCand.p, st};
    if (long_mode) { O.draft_min = cd.u32(c_dmin); HIP_TRY(hypo::arms_long_draftmin(I, O, st)); }
    O.reg_flags = wk.u32(w_flags); O.reg_valid = wk.u32(w_valid); O.reg_counts = wk.at<uint4>(w_counts); O.reg_arms = wk.u32(w_arms); O.reg_bytes = wk.u32(w_bytes);
    O.reg_bytes_int = wk.u32(w_bint); O.reg_bytes_pre = wk.u32(w_bpre); O.reg_draft_bytes = wk.u32(w_dbytes); O.reg_slot = wk.u32(w_slot); O.reg_arm_off = wk.u64(w_armoff);
    O.reg_byte_off = wk.u64(w_byteoff); O.reg_draft_off = wk.u64(w_droff); O.reg_slot_off = wk.u64(w_slotoff); O.win_index = wk.u32(w_widx);
    HIP_TRY(hypo::arms_phase2(I, wk.u32(w_bind), wk.u32(w_nt), wk.u64(w_toff), cd.u32(c_bp), cd.at<uint2>(c_cand), O, st));
    uint64_t* bsum = wk.u64(w_bsum);
    HIP_TRY(hypo::scan32(O.reg_valid, nr, wk.u64(w_winoff), bsum, tot + 1, st));
    HIP_TRY(hypo::scan32(O.reg_arms, nr, wk.u64(w_armoff), bsum, tot + 2, st));
    HIP_TRY(hypo::scan32(O.reg_bytes, nr, wk.u64(w_byteoff), bsum, tot + 3, st));
    HIP_TRY(hypo::scan32(O.reg_draft_bytes, nr, wk.u64(w_droff), bsum, tot + 4, st));
    HIP_TRY(hypo::scan32(O.reg_slot, nr, wk.u64(w_slotoff), bsum, tot + 5, st));
    HIP_TRY(hipMemcpyAsync(h_tot, tot, 64, hipMemcpyDeviceToHost, st));
    std::vector<uint32_t> valid32(nr);
    HIP_TRY(hipMemcpyAsync(valid32.data(), O.reg_valid, (size_t)nr * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (uint32_t i = 0; i < nr; ++i) region_valid[i] = (uint8_t)valid32[i];
    const uint64_t n_win = h_tot[1], n_arms = h_tot[2], arm_bytes = h_tot[3], draft_bytes = h_tot[4], slot_bytes = h_tot[5];
    if (n_arms > 0xfff00000ull || n_win > 0x7fffffffull)
        return fail(HYPO_E_CAPACITY, "%llu windows / %llu arms exceed the 32-bit counters of the boundary", (unsigned long long)n_win, (unsigned long long)n_arms);
    // the batch
    Carver cb;
    const size_t b_win = cb.take(n_win * sizeof(HypoWindow)), b_wreg = cb.take(n_win * 4), b_alen = cb.take(n_arms * 4), b_aoff = cb.take(n_arms * 8),
                 b_arms2 = cb.take(arm_bytes + 16), b_draft = cb.take(draft_bytes + 16), b_ooff = cb.take((n_win + 1) * 8);
    HIP_TRY(dBatch.alloc(cb.at));
    const DevAt bt{(char*)dBatch.p, st};
    O.windows = bt.at<HypoWindow>(b_win); O.win_region = bt.u32(b_wreg); O.arm_len = bt.u32(b_alen); O.arm_off = bt.u64(b_aoff); O.arms2 = bt.u8(b_arms2); O.draft4 = bt.u8(b_draft); O.out_off = bt.u64(b_ooff);
    if (n_win) {
        HIP_TRY(hypo::arms_phase3(I, wk.u32(w_bind), wk.u32(w_nt), wk.u64(w_toff), cd.at<uint2>(c_cand), O, wk.u64(w_winoff), st));
        HIP_TRY(hipMemcpyAsync(O.out_off + n_win, tot + 5, 8, hipMemcpyDeviceToDevice, st));
    }
    sum->n_windows = (uint32_t)n_win; sum->n_arms = (uint32_t)n_arms; sum->arms2_bytes = arm_bytes; sum->draft4_bytes = draft_bytes; sum->out_bytes = slot_bytes;
    AS.sum = *sum; AS.out = O; AS.ready = true;
    return HYPO_OK;
}
int hypo_gpu_arms_build(const HypoArmsRegions* R, const HypoArmsReads* A, uint8_t* region_valid, HypoArmsSummary* sum) { return arms_build_impl(0, R, A, region_valid, sum); }
int hypo_gpu_arms_build_long(const HypoArmsRegions* R, const HypoArmsReads* A, uint8_t* region_valid, HypoArmsSummary* sum) { return arms_build_impl(1, R, A, region_valid, sum); }

static int check_batch(int which) {                   // download and POA need what hypo_gpu_arms_build (which = 0) / _long (1) left on the device
    return g_ctx.arms[which].ready ? HYPO_OK : fail(HYPO_E_INVALID, "no resident batch: call hypo_gpu_arms_build%s first", which ? "_long" : "");
}

static int arms_download_impl(int which, HypoWindow* windows, uint32_t* win_region, uint32_t* arm_len, uint64_t* arm_off, uint8_t* arms2, uint8_t* draft4) {
    HYPO_ENTRY();
    if (const int rc = check_batch(which)) return rc;
    auto& AS = g_ctx.arms[which];
    const HypoArmsSummary& S = AS.sum; const hypo::ArmsOut& O = AS.out;
    hipStream_t st = g_ctx.stream;
    if (windows && S.n_windows) HIP_TRY(hipMemcpyAsync(windows, O.windows, (size_t)S.n_windows * sizeof(HypoWindow), hipMemcpyDeviceToHost, st));
    if (win_region && S.n_windows) HIP_TRY(hipMemcpyAsync(win_region, O.win_region, (size_t)S.n_windows * 4, hipMemcpyDeviceToHost, st));
    if (arm_len && S.n_arms) HIP_TRY(hipMemcpyAsync(arm_len, O.arm_len, (size_t)S.n_arms * 4, hipMemcpyDeviceToHost, st));
    if (arm_off && S.n_arms) HIP_TRY(hipMemcpyAsync(arm_off, O.arm_off, (size_t)S.n_arms * 8, hipMemcpyDeviceToHost, st));
    if (arms2 && S.arms2_bytes) HIP_TRY(d2h(arms2, O.arms2, S.arms2_bytes, st));
    if (draft4 && S.draft4_bytes) HIP_TRY(hipMemcpyAsync(draft4, O.draft4, S.draft4_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return HYPO_OK;
}

int hypo_gpu_arms_download(HypoWindow* windows, uint32_t* win_region, uint32_t* arm_len, uint64_t* arm_off, uint8_t* arms2, uint8_t* draft4) {
    return arms_download_impl(0, windows, win_region, arm_len, arm_off, arms2, draft4);
}
int hypo_gpu_arms_download_long(HypoWindow* windows, uint32_t* win_region, uint32_t* arm_len, uint64_t* arm_off, uint8_t* arms2, uint8_t* draft4) {
    return arms_download_impl(1, windows, win_region, arm_len, arm_off, arms2, draft4);
}

static int arms_poa_impl(int which, const HypoScoreParams* scores, char* bases, uint64_t* off, uint32_t* len, uint8_t* status) {
    HYPO_ENTRY();
    if (const int rc = check_scores(scores)) return rc;
    if (const int rc = check_batch(which)) return rc;
    auto& AS = g_ctx.arms[which];
    const HypoArmsSummary& S = AS.sum; const hypo::ArmsOut& O = AS.out;
    memset(&tl_stats, 0, sizeof(tl_stats));
    const uint32_t n = S.n_windows;
    if (!n) return HYPO_OK;
    if (!bases || !off || !len || !status) return fail(HYPO_E_INVALID, "NULL buffer");
    hipStream_t st = g_ctx.stream;
    DevBuf& dOut = AS.arena[4];
    Carver co;
    // SHORT windows only: the HBM-scratch classes see the odd escalated window, their smallest scratch (16 resident groups) will do;
    // LONG windows: one resident group per window up to what the device holds
    const size_t wsb = hypo::poa_workspace_bytes(n, which ? (int)(n + 64 < 2048u ? n + 64 : 2048u) : hypo::kMinGlobalGroups, 0);
    const size_t o_bases = co.take(S.out_bytes + 16), o_len = co.take((size_t)n * 4), o_st = co.take(n), o_ws = co.take(wsb);
    const bool timing = getenv("HYPO_HOST_TIMING") != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(dOut.alloc(co.at));
    const auto t1 = std::chrono::steady_clock::now();
    char* ob = (char*)dOut.p;
    HIP_TRY(hipMemsetAsync(ob + o_bases, 0, S.out_bytes + 16, st));
    HypoWindowBatch din;
    din.n_windows = n; din.n_arms = S.n_arms; din.windows = O.windows; din.draft4 = O.draft4; din.draft4_bytes = S.draft4_bytes;
    din.arm_off = O.arm_off; din.arm_len = O.arm_len; din.arms2 = O.arms2; din.arms2_bytes = S.arms2_bytes;
    HypoConsensusBatch dout;
    dout.bases = ob + o_bases; dout.off = O.out_off; dout.len = (uint32_t*)(ob + o_len); dout.status = (uint8_t*)(ob + o_st);
    hypo::PoaParams P = make_params(scores, &din, &dout);
    g_ctx.slots[0].aux.next_kind = which;                      // (a LONG batch says nothing about the SHORT one behind it, and the other way round)
    const hipError_t pr = hypo::poa_run(P, n, ob + o_ws, wsb, g_ctx.num_cus, st, nullptr, &g_ctx.slots[0].aux);
    g_ctx.slots[0].aux.next_kind = 0;
    HIP_TRY(pr);
    if (timing) HIP_TRY(hipStreamSynchronize(st));
    const auto t2 = std::chrono::steady_clock::now();
    HIP_TRY(d2h(bases, ob + o_bases, S.out_bytes, st));
    HIP_TRY(hipMemcpyAsync(off, O.out_off, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(len, ob + o_len, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(status, ob + o_st, n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&tl_stats, ob + o_ws + 128, sizeof(HypoPoaStats), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (timing) {
        auto d = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double>(b - a).count() * 1e3; };
        fprintf(stderr, "[timing] hypo_gpu_arms_poa: device buffers (%zu MB) %.2f ms, kernels %.2f ms, results to the host %.2f ms\n", co.at >> 20, d(t0, t1), d(t1, t2), d(t2, std::chrono::steady_clock::now()));
    }
    tl_stats.n_windows = n;
    return HYPO_OK;
}
int hypo_gpu_arms_poa(const HypoScoreParams* scores, char* bases, uint64_t* off, uint32_t* len, uint8_t* status) { return arms_poa_impl(0, scores, bases, off, len, status); }
int hypo_gpu_arms_poa_long(const HypoScoreParams* scores, char* bases, uint64_t* off, uint32_t* len, uint8_t* status) { return arms_poa_impl(1, scores, bases, off, len, status); }

}  // extern "C"
