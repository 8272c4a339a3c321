// Hypo.hpp — host mirror of hypo::Hypo (reference: include/Hypo.hpp:37-58, src/Hypo.cpp:37-329): phase sequencing of
// one polishing run.  Same phases and log labels; polish() is the list of them.  Once per run: the solid k-mers (built from
// the short reads on the device, or loaded), the contigs, their solid positions (Contig::find_solid_pos -> hypo_gpu_solid_scan),
// the result files.  Per contig batch: the reads are loaded and dealt out to the device contexts (CtxPlan.hpp), the k-mer and
// minimizer support votes are counted and the short and long arms cut on the device (DeviceArms) or by the reference's host
// loops, every valid window is polished ("POA of windows": the resident batches per context, the rest in ONE
// Window::generate_consensus_batch call), and a writer thread files the batch beside the next one.  Then the result files
// take their names (RunOutputs.hpp).
#pragma once
#include <chrono>
#include <condition_variable>
#include <fstream>
#include <memory>
#include <mutex>
#include <thread>
#include <string>
#include <unordered_map>
#include <vector>
#include "Alignment.hpp"
#include "Contig.hpp"
#include "CtxPlan.hpp"
#include "DeviceArms.hpp"
#include "ReadBatch.hpp"
#include "SeqIO.hpp"
#include "Settings.hpp"

namespace hypo {

class RunOutputs;
struct Extras;           // run-wide optional outputs: --vcf, the k-mer set of the reads (ReadKmerSet) and the flags that ask it (Hypo.cpp)
struct Batch;            // the contig batch in hand (Hypo.cpp)
struct WriterJob { uint32_t initial_cid = 0, final_cid = 0; };      // what the writer thread is given by value: the contigs to file

struct PhaseTimes { std::vector<std::pair<std::string, double>> phases; double overall = 0; };

class Hypo {
public:
    explicit Hypo(const InputFlags& flags);
    void polish();
    const PhaseTimes& times() const { return _times; }
    // test hook: windows of every contig after arm filling, as (beg, end, type, ni, np, ns, ne, crc32 of arms)
    void set_region_dump(const std::string& path) { _region_dump = path; }

private:
    const InputFlags _cFlags;
    std::vector<std::unique_ptr<Contig>> _contigs;
    std::unordered_map<std::string, uint32_t> _cname_to_id;
    using AlignmentStore = std::vector<std::vector<std::unique_ptr<Alignment>>>;
    AlignmentStore _alignment_store;
    uint32_t _contig_batch_size = 0;
    std::unique_ptr<SamReader> _sf_short, _sf_long;
    // per alignment file: the block of raw records being consumed (a contig batch may end in the middle of it), the block a
    // reader thread fetched meanwhile, and whether the file has more
    // One long-lived thread per alignment file that fetches the next block of raw records when asked (BGZF: inflates a run of blocks
    // on its own team of threads, which lives as long as it does: a thread per block had to raise a new team of 64-128 threads 1 300
    // times on the 3 Gbp set).
    struct BlockReader {
        std::thread th; std::mutex mu; std::condition_variable cv;
        SamReader* sf = nullptr; SamReader::RecordBlock* dst = nullptr; size_t max_rec = 0, max_bytes = 0;
        bool pending = false, done = false, quit = false, more = false;
        void start(SamReader* s) {
            sf = s;
            th = std::thread([this] {
                std::unique_lock<std::mutex> lk(mu);
                for (;;) {
                    cv.wait(lk, [this] { return pending || quit; });
                    if (quit) return;
                    lk.unlock();
                    const bool m = sf->read_block(*dst, max_rec, max_bytes);
                    lk.lock();
                    more = m; pending = false; done = true;
                    cv.notify_all();
                }
            });
        }
        void request(SamReader::RecordBlock* d, size_t n, size_t b) {
            std::lock_guard<std::mutex> lk(mu);
            dst = d; max_rec = n; max_bytes = b; pending = true; done = false;
            cv.notify_all();
        }
        bool wait() { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [this] { return done; }); done = false; return more; }
        ~BlockReader() { { std::lock_guard<std::mutex> lk(mu); quit = true; cv.notify_all(); } if (th.joinable()) th.join(); }
    };
    struct RecordStream {
        std::unique_ptr<BlockReader> reader;
        SamReader::RecordBlock cur, ahead; size_t pos = 0; bool have_ahead = false, more = true;
        // flat path (short reads): the parsed form of `cur`, how far it has been consumed, and the one record a call consumed for
        // a contig of a later batch (the reference files it in that contig's store entry, src/Hypo.cpp:314-325)
        std::shared_ptr<ParsedBlock> parsed; size_t ppos = 0;
        std::shared_ptr<ParsedBlock> carry_blk; size_t carry_r0 = 0, carry_r1 = 0; int32_t carry_cid = -1;
        int32_t opened_with_cid = -1;      // the batch loaded last began with the record carried over from the call before, of this contig (-1: it did not)
    };
    RecordStream _rs_short, _rs_long;
    PhaseTimes _times;
    std::string _region_dump;
    std::chrono::steady_clock::time_point _t0, _tstart;

    void start() { _t0 = std::chrono::steady_clock::now(); }
    void stop(const char* label);
    // Round 4: the short reads of a contig batch as flat slices (ReadBatch.hpp) instead of one Alignment object per record
    ReadBatch _reads;
    ReadBatch _reads_long;                   // the long reads of the batch in hand (-B), flat as well
    std::vector<std::shared_ptr<ParsedBlock>> _block_pool; std::mutex _pool_mu;
    void create_alignments_flat(uint32_t batch_id, ReadBatch& into, bool is_sr = true);
    // long_reads: the normalised-edit-distance filter of the long-read constructor applies (src/Alignment.cpp:51-58)
    void parse_block(const SamReader& sf, const SamReader::RecordBlock& raw, ParsedBlock& blk, bool long_reads);
    // Alignment objects of contigs [c0, c1) of the batch from _reads into _alignment_store (the host loops of the reference read those)
    void materialize_alignments(Batch& b, uint32_t c0, uint32_t c1);

    // ---- polish(), phase by phase ----
    // run-wide state: the teams beside the main thread, the helper threads and what they fill, one DeviceArms per device context
    uint32_t _num_batches = 0;
    int _inflate_threads = 1, _helper_threads = 1, _n_ctx = 1;
    bool _prefetch_on = true;
    std::thread _prefetch, _long_release, _writer;
    ReadBatch _staged;                       // the next batch's short reads while the helper parses them
    std::vector<std::unique_ptr<DeviceArms>> _device_arms;
    std::ofstream _dump;
    // once per run
    void bind_extras(Extras& ex);
    void solid_kmers(Extras& ex, std::ofstream& stagefile, SolidKmers& sk);
    void load_contigs();
    void start_readers();
    void scan_solid_positions(const SolidKmers& sk);
    void open_outputs(Extras& ex, RunOutputs& out);
    // per batch
    void load_reads(Batch& b);
    void plan_batch(Batch& b);
    void kmer_votes(Batch& b);
    void prepare_division(Batch& b);
    void minimizer_votes(Batch& b);
    void divide(Batch& b);
    void cut_short_arms(Batch& b);
    void cut_long_arms(Batch& b);
    void run_poa(Batch& b);
    void dump_regions(const Batch& batch);
    void write_batch(WriterJob job, Extras& ex, RunOutputs& out);          // (the writer thread)
    // once more per run
    void commit_outputs(Extras& ex, RunOutputs& out);
    // what the phases share
    [[noreturn]] void piece_failed(const Batch& b, int d, const char* what);
    template <class F> void contigs_side_by_side(const Batch& b, F per_contig);
    template <class Dev, class Host> void support_votes(Batch& b, const char* what, int kind, Dev on_device, Host per_alignment);
    void widen_piece_halo(int d, const Contig& ctg, bool long_windows);
};

}  // namespace hypo
