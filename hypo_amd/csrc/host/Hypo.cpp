// Hypo.cpp — orchestration of one polishing run (reference: src/Hypo.cpp).
#include "Hypo.hpp"
#include "RunOutputs.hpp"
#include "SolidBuild.hpp"
#include "EditVcf.hpp"
#include "KmerGuard.hpp"
#include "KmerBridge.hpp"
#include "KmerFix.hpp"
#include "KmerSetFile.hpp"
#include "QvReport.hpp"
#include "ReadKmerSet.hpp"
#include "SpectraReport.hpp"
#include "CnReport.hpp"
#include <ctime>
#include <omp.h>
#include <sys/resource.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <atomic>
namespace hypo {
extern std::atomic<uint64_t> g_stage_counters[5];      // host/Contig.cpp

// --vcf, --qv, --qv-bed, --qv-spectra, --qv-cn, --kmer-guard, --kmer-fix, --kmer-bridge: the entry points Hypo::bind_extras bound and what they keep from the reads to the last contig
struct Extras {
    EditScriptsFn edit_fn = nullptr, guard_edit_fn = nullptr;
    ReadKmerSet set;                                       // the k-mers of the reads, on context 0 from bind_extras to commit_outputs
    QvReport qv{set};
    KmerGuard guard{set};
    SpectraReport spectra{set};
    KmerFix fix{set};
    KmerBridge bridge{set};
    CnReport cn{set};
    bool qv_on = false, bed_on = false, guard_on = false, spectra_on = false, fix_on = false, bridge_on = false, vote_on = false, cn_on = false;
    uint32_t min_given = 1;                                // --qv-min-count: 1 = off, 0 = the valley
    bool min_on() const { return min_given != 1; }
    bool ask_on = false;                                   // --qv or --qv-bed: every contig's texts are put to the set
    bool text_on = false;                                  // ... or --qv-spectra or --qv-cn: every contig's texts are needed as strings
    bool set_on = false;                                   // ... or --kmer-guard, --kmer-fix, --kmer-bridge or --qv-save: the set is built
    std::string save_to, load_from;                        // --qv-save / --qv-load: the set also goes to a file / comes from one, not from the reads
    bool save_on() const { return !save_to.empty(); }
    bool load_on() const { return !load_from.empty(); }
    ReadSink set_sink;                                     // (holds a pointer to set: an Extras stays where it is)
    VcfStats vstats;
    Extras() = default; Extras(const Extras&) = delete;
    [[noreturn]] void set_fail(const char* what) {
        std::fprintf(stderr, "[Hypo::QV] Error: %s: %s\n", what, hypo_gpu_last_error());
        set.end();
        std::exit(1);
    }
    // one contig's two texts to whoever wants them: the set's queries, then the marks of --qv-spectra
    int texts(size_t contig, const std::string& draft, const std::string& polished) {
        const int rc = ask_on ? qv.push(contig, draft, polished) : HYPO_OK;
        if (rc == HYPO_OK && cn_on) cn.push(contig, polished);                    // (kept until the last contig: CnReport::run)
        return rc == HYPO_OK && spectra_on ? spectra.push(draft, polished) : rc;
    }
    int texts_flush() {
        const int rc = ask_on ? qv.flush() : HYPO_OK;
        return rc == HYPO_OK && spectra_on ? spectra.flush() : rc;
    }
    [[noreturn]] void set_file_fail(const char* flag, const std::string& why) {
        std::fprintf(stderr, "[Hypo::QV] Error: %s: %s\n", flag, why.c_str());
        set.end();
        std::exit(1);
    }
    // --qv-load: the set comes from the file, where the reads would have been parsed for it.  Every block goes through
    // hypo_gpu_kset_import; then the file's digest must be the sum those calls returned and its n_keys what hypo_gpu_kset_size says.
    void set_load() {
        const auto t0 = std::chrono::steady_clock::now();
        KmerSetFileHeader h;
        std::string err;
        uint64_t in_file = 0, imported = 0;
        int rc = 0;
        auto block = [&](const uint64_t* keys, const uint8_t* counts, uint64_t n) { return set.import_records(keys, counts, n, &imported); };
        if (!read_kmer_set_file(load_from, block, h, in_file, err, rc)) set_file_fail("--qv-load", rc ? err + ": " + hypo_gpu_last_error() : err);
        char why[160];
        if (imported != in_file) {
            std::snprintf(why, sizeof why, ": digest mismatch: the file states %016llx, its records give %016llx", (unsigned long long)in_file, (unsigned long long)imported);
            set_file_fail("--qv-load", load_from + why);
        }
        if (set.reads_done() != HYPO_OK) set_fail("hypo_gpu_kset_size");
        if (set.n_distinct() != h.n_keys) {
            std::snprintf(why, sizeof why, ": size mismatch: the file states %llu k-mers, the set holds %llu", (unsigned long long)h.n_keys, (unsigned long long)set.n_distinct());
            set_file_fail("--qv-load", load_from + why);
        }
        const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        std::fprintf(stdout, "[Hypo::Hypo] Info: k-mer set loaded from %s (k = %u, %llu distinct k-mers, %.3f s)\n", load_from.c_str(), set.k(),
                     (unsigned long long)set.n_distinct(), s);
        set_ready();
        std::fprintf(stderr, "[Hypo::QV] Info: k-mer set of the reads (k = %u): %llu distinct k-mers, from %s (no read parsed for it)\n", set.k(),
                     (unsigned long long)set.n_distinct(), load_from.c_str());
    }
    void set_reads_done(const SolidBuildStats& st, bool shared_pass) {
        if (set.reads_done() != HYPO_OK) set_fail("hypo_gpu_kset_size");
        // --qv-save: the last read is in; every k-mer goes to the file, whatever the least count below is going to be
        if (save_on()) {
            const auto t0 = std::chrono::steady_clock::now();
            std::string err;
            uint64_t bytes = 0;
            int rc = 0;
            auto next = [&](uint64_t* cursor, uint64_t* keys, uint8_t* counts, uint64_t cap, uint64_t* n_out, uint64_t* digest) {
                return set.export_records(cursor, keys, counts, cap, n_out, digest);
            };
            if (!write_kmer_set_file(save_to, set.k(), set.n_distinct(), next, bytes, err, rc)) set_file_fail("--qv-save", rc ? err + ": " + hypo_gpu_last_error() : err);
            const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            std::fprintf(stdout, "[Hypo::Hypo] Info: k-mer set saved to %s (k = %u, %llu distinct k-mers, %llu bytes, %.3f s)\n", save_to.c_str(), set.k(),
                         (unsigned long long)set.n_distinct(), (unsigned long long)bytes, s);
        }
        set_ready();
        std::fprintf(stderr, "[Hypo::QV] Info: k-mer set of the reads (k = %u): %llu distinct k-mers, %.3f s in the insert calls of %.3f GB%s\n", set.k(),
                     (unsigned long long)set.n_distinct(), st.sink_s, st.seq_bytes / 1e9, shared_pass ? " (the parse pass of the solid k-mers)" : " (reads parsed for the QV alone)");
    }
    // the set holds its last k-mer, from the reads or from a file
    void set_ready() {
        // --qv-min-count: the last read is in and nothing has been asked yet; from here on the set answers for the reliable k-mers
        if (min_on()) {
            if (set.set_min_count(min_given) != HYPO_OK) set_fail("hypo_gpu_kset_spectrum / hypo_gpu_kset_min_count");
            std::fprintf(stdout, "[Hypo::Hypo] Info: k-mer min count (k = %u): >= %u (%s), %llu of %llu read k-mers reliable\n", set.k(), set.min_count(),
                         min_given ? "given" : "valley", (unsigned long long)set.n_reliable(), (unsigned long long)set.n_distinct());
        }
    }
};

// one contig batch on its way through the phases of Hypo::polish
struct Batch {
    const uint32_t batch_id, initial_cid, final_cid;
    const bool over_contigs;                               // at least one contig per thread
    Batch(uint32_t id, uint32_t c0, uint32_t c1, bool over) : batch_id(id), initial_cid(c0), final_cid(c1), over_contigs(over) {}
    std::vector<CtxWork> work;                             // per device context: its contigs, or its piece of one
    std::vector<char> votes_dev;                           // per context: its reads are resident
    std::vector<char> on_dev;                              // per contig of the batch: its short arms were cut on a device
    std::vector<char> long_dev;                            // ... and its long arms (LONG windows resident on the device)
    std::vector<char> materialized;                        // per contig of the batch: its Alignment objects exist (host loops)
    int32_t opened_with_cid = -1;
    bool require_device = false;
    std::thread long_prefetch;
    uint32_t n_contigs() const { return final_cid - initial_cid; }
};

namespace {
void host_fallback(const Batch& b, const char* what) {
    if (!b.require_device) return;
    std::fflush(stdout);
    std::fprintf(stderr, "[Hypo::Hypo] Error: --require-device: %s would be computed on the host (last device message: %s)\n", what, hypo_gpu_last_error());
    std::exit(1);
}
// (the main thread may be inside a device call: leave without running the static destructors under it)
[[noreturn]] void writer_fatal(const char* what) {
    std::fprintf(stderr, "[Hypo::Hypo] Error: %s: %s\n", what, hypo_gpu_last_error());
    std::fflush(nullptr);
    RunOutputs::discard();
    std::_Exit(1);
}
// What a flag needs of the device library: an entry point or a group of them as the error line names it (with the blank, comma or
// "and" in front of it), and whether the library has it.  The run ends when one is absent; the line names all of them, or
// (only_absent) the absent ones.
struct Needed { std::string named; bool present; };
void require(const char* flag, std::initializer_list<Needed> needs, bool only_absent = false) {
    std::string absent, all;
    for (const Needed& n : needs) { all += n.named; if (!n.present) absent += n.named; }
    if (absent.empty()) return;
    std::fprintf(stderr, "[Hypo::Hypo] Error: %s needs%s, which the device library does not provide\n", flag, (only_absent ? absent : all).c_str());
    std::exit(1);
}
}

Hypo::Hypo(const InputFlags& flags) : _cFlags(flags) {
    omp_set_num_threads((int)_cFlags.threads);
    _tstart = std::chrono::steady_clock::now();
}

// slog::Monitor::stop prints wall time and RSS per phase (external/slog/src/Monitor.cpp:31-65); same shape of line
void Hypo::stop(const char* label) {
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - _t0).count();
    struct rusage ru; getrusage(RUSAGE_SELF, &ru);
    std::fprintf(stdout, "RESOURCES (%s): TIME= %g sec; PEAK RSS (so far)= %ldMB.\n", label, s, ru.ru_maxrss / 1024);
    _times.phases.emplace_back(label, s);
}

void Hypo::polish() {
    Extras ex;
    bind_extras(ex);
    std::ofstream stagefile(HYPO_STAGEFILE, std::ofstream::out | std::ofstream::app);
    if (_cFlags.intermed && !stagefile.is_open()) {
        std::fprintf(stderr, "[Hypo::Hypo] Error: File open error: Stage File (%s) exists but could not be opened!\n", HYPO_STAGEFILE);
        std::exit(1);
    }
    SolidKmers sk; sk.k = _cFlags.k;
    solid_kmers(ex, stagefile, sk);
    load_contigs();
    start_readers();
    scan_solid_positions(sk);
    RunOutputs out;
    open_outputs(ex, out);
    for (uint32_t batch_id = 0; batch_id < _num_batches; ++batch_id) {
        std::fprintf(stdout, "********** [Hypo::Hypo] Info: BATCH-ID: %u\n", batch_id);
        const uint32_t initial_cid = batch_id * _contig_batch_size;
        const uint32_t final_cid = std::min<uint32_t>((uint32_t)_contigs.size(), initial_cid + _contig_batch_size);
        Batch b(batch_id, initial_cid, final_cid, (final_cid - initial_cid) >= _cFlags.threads);
        load_reads(b);
        plan_batch(b);
        kmer_votes(b);
        prepare_division(b);
        minimizer_votes(b);
        divide(b);
        cut_short_arms(b);
        if (!_cFlags.lr_bam_filename.empty()) cut_long_arms(b);
        else Contig::set_no_long_reads();
        run_poa(b);
        if (_dump.is_open()) dump_regions(b);
        // --vcf: the writer thread aligns the batch's replacement units against their drafts (one call on context 0, beside the
        // next batch's stages on this thread) and formats each contig's records next to its FASTA record, before the contig's
        // windows go
        if (_writer.joinable()) _writer.join();
        _writer = std::thread([this, job = WriterJob{initial_cid, final_cid}, &ex, &out] { write_batch(job, ex, out); });
    }
    _alignment_store.clear();
    if (_long_release.joinable()) _long_release.join();
    commit_outputs(ex, out);
    _times.overall = std::chrono::duration<double>(std::chrono::steady_clock::now() - _tstart).count();
    std::fprintf(stdout, "RESOURCES ([Hypo:Hypo]: Overall. ): TIME= %g sec.\n", _times.overall);
    if (std::getenv("HYPO_STAGE_COUNTERS"))
        std::fprintf(stdout, "[Hypo::Hypo] Info: stage counters: solid k-mers accepted with 40-80 %% support %llu, refused after another such k-mer %llu; force_divide calls %llu; "
                             "minimizers dropped as recurring %llu, as poly-base %llu\n", (unsigned long long)g_stage_counters[0].load(), (unsigned long long)g_stage_counters[1].load(),
                     (unsigned long long)g_stage_counters[2].load(), (unsigned long long)g_stage_counters[3].load(), (unsigned long long)g_stage_counters[4].load());
    // (1.5 M windows with their arms and consensus strings: freed contig by contig on all threads, 0.37 s of the C3 run's wall otherwise)
#pragma omp parallel for schedule(dynamic, 1)
    for (int64_t i = 0; i < (int64_t)_contigs.size(); ++i) _contigs[(size_t)i].reset();
    _contigs.clear();
    _device_arms.clear();
}

// ---- once per run, before the batches ----------------------------------------------------------------------------------------
void Hypo::bind_extras(Extras& ex) {
    ex.fix_on = !_cFlags.kmer_fix_filename.empty();
    ex.bridge_on = !_cFlags.kmer_bridge_filename.empty();
    ex.min_given = _cFlags.qv_min_count;
    ex.spectra_on = !_cFlags.qv_spectra_filename.empty();
    ex.bed_on = !_cFlags.qv_bed_filename.empty();
    ex.guard_on = _cFlags.kmer_guard;
    ex.qv_on = !_cFlags.qv_filename.empty();
    ex.ask_on = ex.qv_on || ex.bed_on;
    ex.cn_on = !_cFlags.qv_cn_filename.empty();
    ex.text_on = ex.ask_on || ex.spectra_on || ex.cn_on;
    ex.save_to = _cFlags.qv_save_filename;
    ex.load_from = _cFlags.qv_load_filename;
    ex.set_on = ex.text_on || ex.guard_on || ex.fix_on || ex.bridge_on || ex.save_on();
    // Every entry point behind these flags is bound by name, and only under its flag, so that libraries without it still serve every
    // run without the flag.  The flags are checked in this order, and each one's error names what it needs.
    const bool have_set = (ex.set_on || ex.min_on()) && ex.set.bind();
    const std::string the_set = ReadKmerSet::kNames;
    // --qv-save: the export of the set's records, and counts on the set so that the file serves every later flag
    if (ex.save_on()) {
        (void)ex.set.bind_counts();
        require("--qv-save", {{" hypo_gpu_kset_export", ex.set.bind_export()}, {" hypo_gpu_kset_counts_enable", ex.set.have_counts()}, {" " + the_set, have_set}}, true);
    }
    // --qv-load: the import of records; the file's header is read now, so that a file that cannot serve ends the run before any stage
    uint64_t load_keys = 0;
    if (ex.load_on()) {
        require("--qv-load", {{" hypo_gpu_kset_import", ex.set.bind_import()}, {" " + the_set, have_set}}, true);
        KmerSetFileHeader h;
        std::string err;
        if (!read_kmer_set_header(ex.load_from, h, err)) { std::fprintf(stderr, "[Hypo::QV] Error: --qv-load: %s\n", err.c_str()); std::exit(1); }
        if (h.k != _cFlags.qv_k) {
            std::fprintf(stderr, "[Hypo::QV] Error: --qv-load: %s: the file holds k-mers of k = %u, --qv-k is %u\n", ex.load_from.c_str(), h.k, _cFlags.qv_k);
            std::exit(1);
        }
        load_keys = h.n_keys;
    }
    // --kmer-bridge-vote: the walk-sets query, and counts on the set it asks
    ex.vote_on = ex.bridge_on && _cFlags.kmer_bridge_vote != 0;
    if (ex.vote_on) {
        (void)ex.set.bind_counts();
        require("--kmer-bridge-vote", {{" hypo_gpu_kset_query_walk_sets", ex.bridge.bind_vote()}, {" hypo_gpu_kset_counts_enable", ex.set.have_counts()}, {" " + the_set, have_set}}, true);
        ex.bridge.configure_vote(_cFlags.kmer_bridge_vote);
    }
    // --kmer-bridge: the walks query and the track query, and the set they ask
    if (ex.bridge_on) {
        require("--kmer-bridge", {{" hypo_gpu_kset_query_walks", ex.bridge.bind()}, {" hypo_gpu_kset_query_track", ex.set.bind_track()}, {" " + the_set, have_set}}, true);
        ex.bridge.configure(_cFlags.kmer_bridge_max, _cFlags.kmer_bridge_slack);
    }
    // --kmer-fix: the fixes query and the track query, and the set they ask
    if (ex.fix_on)
        require("--kmer-fix", {{" hypo_gpu_kset_query_fixes", ex.fix.bind()}, {" hypo_gpu_kset_query_track", ex.set.bind_track()}, {" " + the_set, have_set}}, true);
    // --qv-min-count: counts on the set and the threshold of its queries (1 is the run without it)
    if (ex.min_on())
        require("--qv-min-count", {{" hypo_gpu_kset_counts_enable, hypo_gpu_kset_spectrum and hypo_gpu_kset_min_count,", ex.set.bind_counts()}, {" and " + the_set, have_set}});
    // --qv-cn: the depth query, counts on the set, and the mark of the final text (--qv-spectra's own when both are given)
    if (ex.cn_on) {
        (void)ex.set.bind_counts();
        require("--qv-cn", {{" hypo_gpu_kset_query_depth", ex.set.bind_depth()}, {" hypo_gpu_kset_counts_enable, hypo_gpu_kset_mark and hypo_gpu_kset_spectrum", ex.cn.bind() && ex.set.have_counts()},
                            {" " + the_set, have_set}}, true);
        ex.cn.configure(_cFlags.qv_cn_bin, _cFlags.qv_cn_unit, ex.spectra_on ? (uint32_t)SpectraReport::POLISHED : 0u, !ex.spectra_on);
    }
    // --qv-spectra: counts on the set, and the marks
    if (ex.spectra_on) {
        (void)ex.set.bind_counts();
        require("--qv-spectra", {{" hypo_gpu_kset_counts_enable, hypo_gpu_kset_mark and hypo_gpu_kset_spectrum,", ex.spectra.bind() && ex.set.have_counts()}, {" and " + the_set, have_set}});
    }
    // --qv-bed: the track query, and the set it asks
    if (ex.bed_on) {
        require("--qv-bed", {{" hypo_gpu_kset_query_track", ex.set.bind_track()}, {" and " + the_set, have_set}});
        ex.qv.keep_track();
    }
    // --kmer-guard: the spans query against the set, and the edit scripts whether or not a VCF is written; --guard-records: the
    // variants query as well
    if (ex.guard_on) {
        if (_cFlags.guard_records) require("--guard-records", {{" hypo_gpu_kset_query_variants", ex.guard.bind_variants(_cFlags.guard_records_max)}});
        ex.guard_edit_fn = bind_edit_scripts();
        require("--kmer-guard", {{" hypo_gpu_kset_query_spans", ex.guard.bind()}, {" " + the_set, have_set}, {" hypo_gpu_edit_scripts", ex.guard_edit_fn != nullptr}}, true);
    }
    // --vcf: the edit scripts (C-ABI 10)
    if (!_cFlags.vcf_filename.empty()) require("--vcf", {{" hypo_gpu_edit_scripts (C-ABI 10)", (ex.edit_fn = bind_edit_scripts()) != nullptr}});
    // --qv: the set and its query (C-ABI 11)
    if (ex.qv_on) require("--qv", {{" hypo_gpu_kset_begin / _add / _size / _query / _end (C-ABI 11)", ex.qv.bind() && have_set}});
    // the set lives on context 0 from here until the last contig is written
    if (ex.set_on) {
        // (sized for one k-mer per genome position; what the read errors add makes it grow.  --qv-load: for the file's k-mers)
        const uint64_t cap = _cFlags.qv_mem_gib > 0 ? (uint64_t)(_cFlags.qv_mem_gib * (double)(1ull << 30)) : 0;
        if (ex.set.begin(_cFlags.qv_k, ex.load_on() ? load_keys : _cFlags.genome_size, cap) != HYPO_OK) ex.set_fail("the k-mer set could not be created");
        ex.set_sink = ex.set.sink();
        // --qv-spectra, --qv-cn, --qv-min-count, --kmer-bridge-vote, --qv-save: the set counts from its first k-mer on, with a plane of copy bytes for each
        // text that is going to be marked (one at the least), and the reads reach it window by window, each once
        if (ex.spectra_on || ex.cn_on || ex.min_on() || ex.vote_on || ex.save_on()) {
            if (ex.set.enable_counts(ex.spectra_on ? SpectraReport::N_TEXTS : 1) != HYPO_OK) ex.set_fail("the k-mer set could not be made to count");
            ex.set_sink.exact = true;
        }
    }
}

// ---- solid k-mers: built from the short reads on the device (stage 0), or loaded from aux/solid_kmers.bvsd ------------------
void Hypo::solid_kmers(Extras& ex, std::ofstream& stagefile, SolidKmers& sk) {
    start();
    if (_cFlags.done_stage < 1) {
        SolidBuildStats st;
        std::string err;
        const int rc = build_solid_kmers(_cFlags.sr_filenames, _cFlags.k, _cFlags.cov, (int)_cFlags.threads, sk, st, err, ex.set_on && !ex.load_on() ? &ex.set_sink : nullptr);
        if (rc == SOLID_E_SINK) { std::fprintf(stderr, "[Hypo::QV] Error: the k-mer set of the reads: %s\n", err.c_str()); ex.set.end(); std::exit(1); }
        if (rc == SOLID_E_UNDEFINED) {                   // the reference's own line for a failed initialise (src/Hypo.cpp:53)
            std::fprintf(stderr, "[Hypo::SolidKmers] Error: %s\n", err.c_str());
            std::fprintf(stderr, "[Hypo::SolidKmers] Error: KMC Output: Could not have successful run of SUK for computing Solid kmers!\n");
            std::exit(1);
        }
        if (rc != SOLID_OK) {
            std::fprintf(stderr, "[Hypo::SolidKmers] Error: %s%s\n", rc == SOLID_E_DEVICE ? "device k-mer counting failed: " : "", err.c_str());
            std::exit(1);
        }
        std::fprintf(stderr, "[Hypo::SolidKmers] Info: device construction: %.3f s (parse %.3f s of %.3f GB, count %.3f s of %.3f GB sent, "
                             "histogram %.3f s, set %.3f s)\n", st.total_s, st.parse_s, st.file_bytes / 1e9, st.count_s, st.seq_bytes / 1e9, st.hist_s, st.fill_s);
        if (ex.set_on && ex.load_on()) ex.set_load();          // (the solid k-mers were counted from the reads, without the sink)
        else if (ex.set_on) ex.set_reads_done(st, true);
        if (_cFlags.intermed) {
            if (!sk.store(HYPO_SKFILE)) {
                std::fprintf(stderr, "[Hypo::SolidKmers] Error: File Saving: Could not store the DS for Solid kmers!\n");
                std::exit(1);
            }
            stop("[Hypo:Hypo]: Computed Solid kmers. ");
            const std::time_t now = std::time(nullptr);
            char tm[32];
            std::strftime(tm, sizeof tm, "%Y-%m-%d %H:%M:%S", std::localtime(&now));
            stagefile << "Stage:SolidKmers [" << tm << "]\t1" << std::endl;
        } else {
            stop("[Hypo:Hypo]: Computed Solid kmers. ");
        }
    } else {
        if (!sk.load(HYPO_SKFILE)) {
            std::fprintf(stderr, "[Hypo::SolidKmers] Error: File Loading: Could not load the DS for Solid kmers (%s)!\n", HYPO_SKFILE);
            std::exit(1);
        }
        if (ex.set_on && ex.load_on()) ex.set_load();    // neither set needs the reads: none is opened
        else if (ex.set_on) {                            // the stored set needs no reads; the QV and the guard do
            SolidBuildStats st;
            std::string err;
            const int rc = stream_reads(_cFlags.sr_filenames, ex.set_sink, st, err);
            if (rc != SOLID_OK) { std::fprintf(stderr, "[Hypo::QV] Error: the k-mer set of the reads: %s\n", err.c_str()); ex.set.end(); std::exit(1); }
            ex.set_reads_done(st, false);
        }
        stop("[Hypo:Hypo]: Loaded Solid kmers. ");
    }
    std::fprintf(stdout, "[Hypo::Hypo] Info: Number of (canonical) solid kmers (nonhp) : %lu\n", (unsigned long)sk.num_solid);
}

// ---- contigs ------------------------------------------------------------------------------------------------------
void Hypo::load_contigs() {
    start();
    {
        std::vector<FastaRecord> recs;
        if (!read_fastx(_cFlags.draft_filename, recs)) {
            std::fprintf(stderr, "[Hypo::Hypo] Error: File open error: Draft File (%s) could not be read!\n", _cFlags.draft_filename.c_str());
            std::exit(1);
        }
        // (the records are packed into Contig objects on all threads: 100 x 1 Mbp took 0.7 s one after the other)
        // (a handful of large contigs: one after the other, each packed by all threads — PackedSeq::assign)
        _contigs.resize(recs.size());
        const bool many = recs.size() >= (size_t)std::max(2u, _cFlags.threads / 2);
#pragma omp parallel for schedule(dynamic, 1) if (many)
        for (int64_t i = 0; i < (int64_t)recs.size(); ++i) {
            _contigs[(size_t)i].reset(new Contig((uint32_t)i, recs[(size_t)i].name, recs[(size_t)i].seq));
            std::string().swap(recs[(size_t)i].seq);
        }
        for (size_t i = 0; i < recs.size(); ++i) _cname_to_id[recs[i].name] = (uint32_t)i;
    }
    stop("[Hypo:Hypo]: Loaded Contigs. ");
    _alignment_store.resize(_contigs.size());
}

// the batches, the short-read file, the teams beside the main thread, and the helper that parses the first batch's short reads
void Hypo::start_readers() {
    _contig_batch_size = _cFlags.processing_batch_size == 0 ? (uint32_t)_contigs.size() : _cFlags.processing_batch_size;
    _num_batches = _contig_batch_size ? (uint32_t)_contigs.size() / _contig_batch_size : 0;
    if (_contig_batch_size && _contigs.size() % _contig_batch_size != 0) ++_num_batches;
    _sf_short.reset(new SamReader(_cFlags.sr_bam_filename));
    if (!_sf_short->ok()) { std::fprintf(stderr, "[Hypo::Hypo] Error: File open error: %s\n", _cFlags.sr_bam_filename.c_str()); std::exit(1); }
    // (a run of ONE batch has nothing beside the parser but the scans: it keeps whole teams)
    const int side_team = _num_batches > 1 ? std::max(1, (int)_cFlags.threads / 2) : std::max(1, (int)_cFlags.threads);
    _inflate_threads = std::getenv("HYPO_INFLATE_THREADS") ? std::max(1, std::atoi(std::getenv("HYPO_INFLATE_THREADS"))) : side_team;
    _sf_short->set_inflate_threads(_inflate_threads);
    // the short reads of the first batch are parsed while the contigs are scanned (the parser needs the contigs' names and lengths only)
    _prefetch_on = !(std::getenv("HYPO_PREFETCH") && std::atoi(std::getenv("HYPO_PREFETCH")) == 0);
    // The parser's team and the team that inflates BGZF blocks for it are HALF of -t each: with all three teams (these two and the main
    // thread's phases) at -t the stages only got in each other's way — 500 Mbp at k = 17, -t 64 on the 128-core box: 4.4-4.8 s with
    // 64 / 64, 3.7-4.0 s with 32 / 32, 3.8 s with 16 / 16 or 24 / 24 (profiles/history/r04_thread_split.txt).
    _helper_threads = side_team;
    if (const char* e = std::getenv("HYPO_HELPER_THREADS")) _helper_threads = std::max(1, std::atoi(e));        // (experiments)
    if (_prefetch_on && _num_batches > 0) {
        _staged.reset(_contigs.size());
        _prefetch = std::thread([this] { omp_set_num_threads(_helper_threads); create_alignments_flat(0, _staged); });
    }
}

// ---- solid positions: device scan (the C-ABI call is serialised on the context's stream) ------
void Hypo::scan_solid_positions(const SolidKmers& sk) {
    // the 4^k-bit set goes to the device once (2 GiB at the default k = 17), not once per contig
    start();
    if (hypo_gpu_solid_set_upload(sk.words.data(), sk.get_k()) != HYPO_OK) { std::fprintf(stderr, "[Hypo::Hypo] Error: %s\n", hypo_gpu_last_error()); std::exit(1); }
    {   // A few contigs side by side: the device part of a scan (copy in, kernel, copy out) runs under the context's lock, one
        // contig at a time; what a thread does around it — fresh pages for 8 bytes per base, the copy into the contig's own
        // vectors — overlaps with the next contig's device part (250 x 1 Mbp at k = 15, nearly every position solid: 1.1 s one
        // after the other)
        const int nt = std::max(1, std::min((int)_cFlags.threads, 4));
#pragma omp parallel for schedule(dynamic, 1) num_threads(nt)
        for (int64_t i = 0; i < (int64_t)_contigs.size(); ++i) {
            if (_contigs[(size_t)i]->find_solid_pos(sk, true) != HYPO_OK) { std::fprintf(stderr, "[Hypo::Contig] Error: %s\n", hypo_gpu_last_error()); std::exit(1); }
        }
    }
    stop("[Hypo:Hypo]: Found Solid pos in contigs. ");
}

// the long-read file, the region dump, one DeviceArms per device context, and the result files
void Hypo::open_outputs(Extras& ex, RunOutputs& out) {
    std::fprintf(stdout, "[Hypo::Hypo] Info: Number.of contigs: %lu; Number of batches: %u\n", (unsigned long)_contigs.size(), _num_batches);
    if (!_cFlags.lr_bam_filename.empty()) {
        _sf_long.reset(new SamReader(_cFlags.lr_bam_filename));
        if (!_sf_long->ok()) { std::fprintf(stderr, "[Hypo::Hypo] Error: File open error: %s\n", _cFlags.lr_bam_filename.c_str()); std::exit(1); }
        _sf_long->set_inflate_threads(_inflate_threads);
    }
    // which inflate path this run takes (libdeflate is bound by name at run time, zlib is the fall-back: the two differ by 1.5 x on a
    // 3 Gbp run, so a number quoted from this binary should say which one it was)
    if (_sf_short->bgzf() || (_sf_long && _sf_long->bgzf()))
        std::fprintf(stdout, "[Hypo::Hypo] Info: BGZF blocks are inflated by %s on %d threads\n", BlockInflater::name(), _inflate_threads);
    if (!_region_dump.empty()) _dump.open(_region_dump);

    // one per device context (they outlive the batches: spent alignments are released behind the phases that follow)
    _n_ctx = std::max(1, hypo_gpu_num_devices());
    for (int d = 0; d < _n_ctx; ++d) _device_arms.emplace_back(new DeviceArms(d));
    _reads.reset(_contigs.size());
    // The polished contigs of a batch are filed by a writer thread while the next batch is processed (the reference writes
    // everything at the end, src/Hypo.cpp:256-268: the same bytes in the same order); what a written contig no longer needs is
    // released there.
    out.open_fasta(_cFlags.output_filename);
    if (ex.edit_fn) vcf_header(out.open_vcf(_cFlags.vcf_filename), _cFlags.draft_filename, _contigs, ex.guard_on);
}

// ---- the phases of a batch ---------------------------------------------------------------------------------------------------
void Hypo::load_reads(Batch& b) {
    // The short-read records of the NEXT batch are parsed on a helper thread while this batch is with the device (support
    // votes, arms and POA leave the host's cores idle most of the time); it fills a store of its own,
    // the reader state belongs to create_alignments alone.  HYPO_PREFETCH=0: one batch after the other.
    start();
    // (records of contigs behind the previous batch that it had consumed — _reads holds them — come first, then what the helper
    // or this thread parses now)
    const size_t slices_before = _reads.n_slices();
    if (_prefetch.joinable()) {
        _prefetch.join();
        _reads.append(_staged);
    } else {
        create_alignments_flat(b.batch_id, _reads);
    }
    // (read before the helper starts on the next batch: did this batch's load open with the record carried over, and of which contig)
    b.opened_with_cid = _rs_short.opened_with_cid;
    stop("[Hypo:Hypo]: Loaded alignments. ");
    if (_prefetch_on && b.batch_id + 1 < _num_batches) {
        _staged.reset(_contigs.size());
        // (the helper's team: all of -t while the machine has threads to spare, half of it otherwise — the main thread's own
        // parallel phases run next to it)
        _prefetch = std::thread([this, batch_id = b.batch_id] { omp_set_num_threads(_helper_threads); create_alignments_flat(batch_id + 1, _staged); });
    }
    // ... and THIS batch's long reads (-B) are read and parsed while its short-read phases run (the reference loads them behind the
    // short arms, src/Hypo.cpp:225-229; what they are does not depend on anything those phases compute): 2.4 of the 8 s of the
    // 250 Mbp set.  The record the long reader consumed for a later contig during the LAST batch is already in that contig's
    // store entry (below), so the order of the two streams is the reference's.
    if (_prefetch_on && !_cFlags.lr_bam_filename.empty()) {
        if (_long_release.joinable()) _long_release.join();
        _reads_long.reset(_contigs.size());
        b.long_prefetch = std::thread([this, batch_id = b.batch_id] { omp_set_num_threads(_helper_threads); create_alignments_flat(batch_id, _reads_long, false); });
    }
    b.materialized.assign(b.n_contigs(), 0);
    // The first long read of a contig may have been consumed while the previous batch's long reads were loaded; the reference
    // files it in this contig's store entry, where the short-read phases of THIS batch find it in front of the short reads and
    // treat it as one of them (src/Hypo.cpp:314-325, :126-199).  Same here: it moves to the front of the flat batch.
    // ... in front of them but for ONE: when the short-read loader of the batch before had already consumed this contig's first short
    // read, that record was filed first (store entry = [short carry, long carry, this batch's short reads ..]): the long read goes
    // behind the batch's opening record then.  Arm order inside a window is record order, and POA depends on it.
    // (the contig the batch opened with goes FIRST: `slices_before + 1` is an index into the slice list as it stands now, and every
    // other contig's records are put in front of everything afterwards, which shifts indices but not the order inside a contig)
    const int32_t opened_with_cid = b.opened_with_cid;
    if (opened_with_cid >= (int32_t)b.initial_cid && opened_with_cid < (int32_t)b.final_cid && !_alignment_store[(size_t)opened_with_cid].empty()) {
        _reads.prepend((uint32_t)opened_with_cid, _alignment_store[(size_t)opened_with_cid], slices_before + 1);
        _alignment_store[(size_t)opened_with_cid].clear();
    }
    for (uint32_t c = b.initial_cid; c < b.final_cid; ++c)
        if (!_alignment_store[c].empty()) { _reads.prepend(c, _alignment_store[c], 0); _alignment_store[c].clear(); }
}

// the contigs of the batch are dealt out to the device contexts (CtxPlan.hpp), and every context is told its piece, if it has one
void Hypo::plan_batch(Batch& b) {
    std::vector<uint64_t> n_reads(b.n_contigs());
    std::vector<uint32_t> contig_len(b.n_contigs());
    for (uint32_t c = b.initial_cid; c < b.final_cid; ++c) { n_reads[c - b.initial_cid] = _reads.count(c); contig_len[c - b.initial_cid] = (uint32_t)_contigs[c]->get_len(); }
    const bool split_batch = (uint32_t)_n_ctx > 1 && !_cFlags.host_arms;
    // (the probe: a library without the resident-read entry points — the CPU test shim — answers HYPO_E_UNSUPPORTED, and the
    // host loops, which know nothing of pieces, take the batch as before)
    const bool allow_pieces = split_batch && b.n_contigs() < (uint32_t)_n_ctx && !std::getenv("HYPO_NO_PIECES") && hypo_gpu_reads_upload(nullptr, nullptr, 0) != HYPO_E_UNSUPPORTED;
    b.work = plan_contexts(b.initial_cid, b.final_cid, _n_ctx, n_reads.data(), contig_len.data(), split_batch, allow_pieces);
    for (int d = 0; d < _n_ctx; ++d) {
        const CtxWork& w = b.work[(size_t)d];
        if (w.piece) {
            // halo: the longest read of the contig + the longest window a read at the edge can still reach into
            const uint32_t halo = _reads.max_span(w.c0) + 2048;
            _device_arms[(size_t)d]->set_piece(w.own0, w.own1, halo, (uint32_t)_contigs[w.c0]->get_len());
            std::fprintf(stdout, "[Hypo::Hypo] Info: context %d owns [%u, %u) of contig %s (halo %u)\n", d, w.own0, w.own1, _contigs[w.c0]->get_name().c_str(), halo);
        } else _device_arms[(size_t)d]->clear_piece();
    }
    (void)hypo_gpu_last_error();
}

void Hypo::piece_failed(const Batch& b, int d, const char* what) {
    std::fprintf(stderr, "[Hypo::Hypo] Error: %s failed on context %d, which shares contig %s with other contexts (%s); run on one device or with --host-arms\n",
                 what, d, _contigs[b.work[(size_t)d].c0]->get_name().c_str(), hypo_gpu_last_error());
    std::exit(1);
}

// One support-vote stage: every context counts the votes of its contigs on the device (on_device), or the reference's host loop
// runs per_alignment over the contigs' Alignment objects.  kind: what Contig::dump_votes calls the counters, 0 = solid k-mers,
// 1 = minimizers.
template <class Dev, class Host> void Hypo::support_votes(Batch& b, const char* what, int kind, Dev on_device, Host per_alignment) {
    for (int d = 0; d < _n_ctx; ++d) {
        const uint32_t c0 = b.work[(size_t)d].c0, c1 = b.work[(size_t)d].c1;
        if (c0 >= c1) continue;
        if (b.votes_dev[(size_t)d] && on_device(*_device_arms[(size_t)d], c0, c1)) continue;
        if (b.work[(size_t)d].piece) piece_failed(b, d, what);
        { uint64_t nr = 0; for (uint32_t c = c0; c < c1; ++c) nr += _reads.count(c); if (nr) host_fallback(b, what); }
        materialize_alignments(b, c0, c1);
        for (uint32_t cid = c0; cid < c1; ++cid) {
            if (kind == 0) _contigs[cid]->ensure_kids();
            auto& alns = _alignment_store[cid];
#pragma omp parallel for
            for (int64_t t = 0; t < (int64_t)alns.size(); ++t) per_alignment(*alns[(size_t)t], *_contigs[cid]);
        }
    }
    hypo_gpu_use_device(0);
    if (const char* vp = std::getenv("HYPO_DUMP_VOTES"))        // (tests: device votes against the host loops of the reference, counter by counter)
        if (std::FILE* vf = std::fopen(vp, kind == 0 && b.batch_id == 0 ? "wb" : "ab")) { for (uint32_t c = b.initial_cid; c < b.final_cid; ++c) _contigs[c]->dump_votes(vf, kind); std::fclose(vf); }
}

void Hypo::kmer_votes(Batch& b) {
    // N1: the reads go to the device once, now; the support votes are counted there (support_kernel.hip) and the arm kernels
    // use the same copy later.  --host-arms, an unsorted file or a device error: the reference's host loops, per contig range.
    start();
    // --require-device / HYPO_REQUIRE_DEVICE=1: a stage that was meant for the device and is about to run in the host loops ends
    // the run instead (the Info lines of DeviceArms say why it did not run there).  Not with --host-arms / HYPO_HOST_SUPPORT,
    // which ask for the host loops.
    b.require_device = (_cFlags.require_device || (std::getenv("HYPO_REQUIRE_DEVICE") && std::atoi(std::getenv("HYPO_REQUIRE_DEVICE")) != 0)) &&
                       !_cFlags.host_arms && !std::getenv("HYPO_HOST_SUPPORT");
    b.votes_dev.assign((size_t)_n_ctx, 0);
    if (!_cFlags.host_arms && !std::getenv("HYPO_HOST_SUPPORT"))
        for (int d = 0; d < _n_ctx; ++d) {
            const uint32_t c0 = b.work[(size_t)d].c0, c1 = b.work[(size_t)d].c1;
            if (c0 < c1) b.votes_dev[(size_t)d] = _device_arms[(size_t)d]->upload_reads(_contigs, c0, c1, _reads) ? 1 : 0;
            if (c0 < c1 && b.work[(size_t)d].piece && !b.votes_dev[(size_t)d]) piece_failed(b, d, "the upload of the reads");
        }
    support_votes(b, "the k-mer support votes", 0, [this](DeviceArms& da, uint32_t c0, uint32_t c1) { return da.support_kmers(_contigs, c0, c1, _cFlags.k); },
                  [this](Alignment& a, Contig& ctg) { a.update_solidkmers_support(_cFlags.k, ctg); });
    stop("[Hypo:Hypo]: Solid kmers support update. ");
}

// many contigs: one contig per thread as in the reference; fewer contigs than threads: the contigs side by side, each
// with its share of the threads for the minimizers of its mega-windows or for building its Window objects (a nested team; -p 10
// on 64 threads took 45 ms per batch one contig after the other)
template <class F> void Hypo::contigs_side_by_side(const Batch& b, F per_contig) {
    const int nc = (int)b.n_contigs(), T = (int)_cFlags.threads;
    const int outer = std::max(1, std::min(nc, T)), inner = b.over_contigs ? 1 : std::max(1, T / outer);
    if (inner > 1) omp_set_max_active_levels(2);
#pragma omp parallel for schedule(static, 1) num_threads(outer)
    for (int64_t i = b.initial_cid; i < (int64_t)b.final_cid; ++i) {
        omp_set_num_threads(inner);
        per_contig(*_contigs[(size_t)i]);
    }
    omp_set_max_active_levels(1);
}

void Hypo::prepare_division(Batch& b) {
    start();
    contigs_side_by_side(b, [this](Contig& ctg) { ctg.prepare_for_division(_cFlags.k); });
    uint64_t num_sr = 0, len_sr = 0;
    for (uint32_t i = b.initial_cid; i < b.final_cid; ++i) { num_sr += _contigs[i]->get_num_sr(); len_sr += _contigs[i]->get_len_sr(); }
    std::fprintf(stdout, "[Hypo::Hypo] Info: Total number of SR: %lu; Total length of SR: %lu\n", (unsigned long)num_sr, (unsigned long)len_sr);
    stop("[Hypo:Hypo]: Finding SR (and preparing for division). ");
}

void Hypo::minimizer_votes(Batch& b) {
    start();
    support_votes(b, "the minimizer support votes", 1, [this](DeviceArms& da, uint32_t c0, uint32_t c1) { return da.support_minimizers(_contigs, c0, c1); },
                  [](Alignment& a, Contig& ctg) { a.update_minimisers_support(ctg); });
    stop("[Hypo:Hypo]: Minimisers support update. ");
}

void Hypo::divide(Batch& b) {
    start();
    contigs_side_by_side(b, [](Contig& ctg) { ctg.divide_into_regions(); });
    stop("[Hypo:Hypo]: Division into windows. ");
}

// The halo of a piece was chosen before the division: a window longer than it (a weak region force_divide could not cut) would lose
// the arms of the reads beyond it — the span grows to the longest window this context owns and its reads go over again.  For the
// long arms likewise, once the LONG pseudo-windows exist.
void Hypo::widen_piece_halo(int d, const Contig& ctg, bool long_windows) {
    DeviceArms& da = *_device_arms[(size_t)d];
    const uint32_t longest = da.longest_owned_window(ctg, long_windows);
    if (da.widen_halo(longest + 64))
        std::fprintf(stdout, long_windows ? "[Hypo::Hypo] Info: context %d owns a LONG window of %u bases: halo widened to %u\n"
                                          : "[Hypo::Hypo] Info: context %d owns a window of %u bases: halo widened to %u, its reads are uploaded again\n", d, longest, da.halo());
}

void Hypo::cut_short_arms(Batch& b) {
    const uint32_t initial_cid = b.initial_cid, final_cid = b.final_cid;
    start();
    // The device cuts the reads into arms, prunes the windows and keeps the window batch in its memory (DeviceArms.hpp);
    // --host-arms, several devices or an unsorted alignment file take the host loops of the reference instead.
    b.on_dev.assign(b.n_contigs(), 0);
    b.long_dev.assign(b.n_contigs(), 0);
    if (!_cFlags.host_arms) {
        for (int d = 0; d < _n_ctx; ++d) {
            const uint32_t c0 = b.work[(size_t)d].c0, c1 = b.work[(size_t)d].c1;
            if (c0 >= c1) continue;
            if (b.work[(size_t)d].piece) widen_piece_halo(d, *_contigs[c0], false);
            if (_device_arms[(size_t)d]->build(_contigs, c0, c1, _reads, _cFlags.k))
                for (uint32_t c = c0; c < c1; ++c) b.on_dev[c - initial_cid] = 1;
            else if (b.work[(size_t)d].piece) piece_failed(b, d, "short-arm selection");
        }
        for (int d = 0; d < _n_ctx; ++d) if (b.work[(size_t)d].piece) DeviceArms::finish_short(_contigs, b.work[(size_t)d].c0, b.work[(size_t)d].c1);
        hypo_gpu_use_device(0);
    }
    for (uint32_t cid = initial_cid; cid < final_cid; ++cid) {
        if (b.on_dev[cid - initial_cid]) { _alignment_store[cid].clear(); continue; }       // (objects a host vote loop had asked for)
        if (!_cFlags.host_arms && _reads.count(cid) > 0) host_fallback(b, "short-arm selection");
        materialize_alignments(b, cid, cid + 1);
        auto& alns = _alignment_store[cid];
#pragma omp parallel for
        for (int64_t t = 0; t < (int64_t)alns.size(); ++t) alns[(size_t)t]->find_short_arms(_cFlags.k, *_contigs[cid]);
    }
    stop("[Hypo:Hypo]: Short arms computing. ");
    start();
    // few contigs: the parallelism is inside a contig (window ranges); many contigs: one contig per thread as in the reference
#pragma omp parallel for schedule(static, 1) if (b.over_contigs)
    for (int64_t i = initial_cid; i < (int64_t)final_cid; ++i) {
        if (b.on_dev[(size_t)i - initial_cid]) continue;
        _contigs[(size_t)i]->fill_short_windows(_alignment_store[(size_t)i]); _alignment_store[(size_t)i].clear();
    }
    {   // the batch's short reads are spent; what it consumed for contigs of later batches stays for them (src/Hypo.cpp:314-325)
        ReadBatch later;
        later.reset(_contigs.size());
        _reads.carry_beyond(final_cid, later);
        _reads.clear(&_block_pool, &_pool_mu);
        _reads.reset(_contigs.size());
        _reads.append(later);
    }
    stop("[Hypo:Hypo]: Short arms filling. ");
}

void Hypo::cut_long_arms(Batch& b) {
    const uint32_t initial_cid = b.initial_cid, final_cid = b.final_cid;
    start();
    // the long reads of the batch, flat like the short ones (ReadBatch.hpp; round 4: 1.2 M objects of 8 kb each took 2.5 s to
    // build on the 250 Mbp set).  The reader stops behind the first kept record of a later contig; the reference files that
    // record in ITS contig's store entry (src/Hypo.cpp:314-325), where that batch's short-read phases find it: it becomes
    // an object there (see Hypo::load_reads).
    if (b.long_prefetch.joinable()) b.long_prefetch.join();
    else { _reads_long.reset(_contigs.size()); create_alignments_flat(b.batch_id, _reads_long, false); }
    if (_rs_long.carry_blk) {
        ReadBatch one;
        one.reset(_contigs.size());
        one.add(_rs_long.carry_blk, _rs_long.carry_r0, _rs_long.carry_r1);
        if (_rs_long.carry_cid >= 0) one.materialize((uint32_t)_rs_long.carry_cid, _alignment_store[(size_t)_rs_long.carry_cid]);
        _rs_long.carry_blk.reset();
    }
    stop("[Hypo:Hypo]: Loaded alignments of Long reads. ");
    start();
    const auto tl0 = std::chrono::steady_clock::now();
#pragma omp parallel for schedule(static, 1)
    for (int64_t i = initial_cid; i < (int64_t)final_cid; ++i) _contigs[(size_t)i]->prepare_long_windows();
    const auto tl1 = std::chrono::steady_clock::now();
    // the long reads are cut into arms, filtered (Filter::is_good) and kept as a second resident batch by the context that
    // holds the contig's short arms; --host-arms, an unsorted file or a device error take the reference's host loops
    std::vector<char> long_on_dev(b.n_contigs(), 0);
    if (!_cFlags.host_arms) {
        for (int d = 0; d < _n_ctx; ++d) {
            const uint32_t c0 = b.work[(size_t)d].c0, c1 = b.work[(size_t)d].c1;
            if (c0 >= c1) continue;
            if (b.work[(size_t)d].piece) widen_piece_halo(d, *_contigs[c0], true);
            if (_device_arms[(size_t)d]->build_long(_contigs, c0, c1, _reads_long))
                for (uint32_t c = c0; c < c1; ++c) long_on_dev[c - initial_cid] |= 1;
            else {
                if (_device_arms[(size_t)d]->long_failed()) host_fallback(b, "long-arm selection");
                if (b.work[(size_t)d].piece) long_on_dev[c0 - initial_cid] |= 2;      // (a shared contig: all of its contexts or none)
            }
        }
        for (int d = 0; d < _n_ctx; ++d) {
            if (!b.work[(size_t)d].piece) continue;
            const uint32_t c = b.work[(size_t)d].c0;
            if (long_on_dev[c - initial_cid] & 2) _device_arms[(size_t)d]->drop_long();
        }
        for (uint32_t c = initial_cid; c < final_cid; ++c) {
            char& f = long_on_dev[c - initial_cid];
            const bool shared = f != 0 && b.n_contigs() < (uint32_t)_n_ctx;
            if (f & 2) f = 0;
            else if (f == 1 && shared) DeviceArms::finish_long(_contigs, c, c + 1);
        }
        hypo_gpu_use_device(0);
    }
    for (uint32_t cid = initial_cid; cid < final_cid; ++cid) {
        if (long_on_dev[cid - initial_cid]) continue;
        auto& alns = _alignment_store[cid];                     // (the host loops of the reference read objects)
        _reads_long.materialize(cid, alns);
#pragma omp parallel for
        for (int64_t t = 0; t < (int64_t)alns.size(); ++t) alns[(size_t)t]->find_long_arms(*_contigs[cid]);
    }
#pragma omp parallel for schedule(static, 1) if (b.over_contigs)
    for (int64_t i = initial_cid; i < (int64_t)final_cid; ++i) {
        if (long_on_dev[(size_t)i - initial_cid]) continue;
        _contigs[(size_t)i]->fill_long_windows(_alignment_store[(size_t)i]); _alignment_store[(size_t)i].clear();
    }
    for (uint32_t c = initial_cid; c < final_cid; ++c) b.long_dev[c - initial_cid] = long_on_dev[c - initial_cid];
    const auto tl2 = std::chrono::steady_clock::now();
    // (7 GB of parsed long reads on the 250 Mbp set: handed back behind the POA, not in front of it)
    if (_long_release.joinable()) _long_release.join();
    _long_release = std::thread([this, spent = std::make_shared<ReadBatch>(std::move(_reads_long))] { spent->clear(&_block_pool, &_pool_mu); });
    _reads_long = ReadBatch();
    if (std::getenv("HYPO_HOST_TIMING")) {
        auto sec = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double>(b - a).count(); };
        std::fprintf(stderr, "[timing] long arms: prepare_long_windows %.3f s, arms %.3f s, long reads released %.3f s\n", sec(tl0, tl1), sec(tl1, tl2), sec(tl2, std::chrono::steady_clock::now()));
    }
    stop("[Hypo:Hypo]: Long arms filling. ");
}

// ---- POA: every valid window of the contig batch in one device call (reference: per-window OpenMP loop) ----
void Hypo::run_poa(Batch& b) {
    const uint32_t initial_cid = b.initial_cid, final_cid = b.final_cid;
    start();
    Window::prepare_for_poa(_cFlags.score_params, _cFlags.threads);
    std::vector<Window*> wins;
    for (uint32_t i = initial_cid; i < final_cid; ++i)
        for (uint64_t w = 0; w < _contigs[i]->get_num_regions(); ++w)
            if (_contigs[i]->is_valid_window((uint32_t)w)) {
                const bool lw = _contigs[i]->window((uint32_t)w)->is_long();
                if (!(lw ? b.long_dev[i - initial_cid] : b.on_dev[i - initial_cid])) wins.push_back(_contigs[i]->window((uint32_t)w));
            }
    uint64_t n_resident = 0;
    {   // the resident batches: every context polishes its own, side by side; what needs the host's retry path joins `wins`
        std::vector<std::vector<Window*>> retry((size_t)_n_ctx);
        std::vector<int> prc((size_t)_n_ctx, HYPO_OK);
        std::vector<std::string> perr((size_t)_n_ctx);
        std::vector<std::thread> th;
        for (int d = 0; d < _n_ctx; ++d) {
            DeviceArms& da = *_device_arms[(size_t)d];
            da.reset_polished();
            if (!da.active() && !da.active_long()) continue;

            auto job = [&, d] {
                DeviceArms& me = *_device_arms[(size_t)d];
                prc[(size_t)d] = me.polish(_cFlags.score_params, _dump.is_open(), &retry[(size_t)d]);
                if (prc[(size_t)d] == HYPO_OK) prc[(size_t)d] = me.polish_long(_cFlags.score_params, _dump.is_open(), &retry[(size_t)d]);
                if (prc[(size_t)d] != HYPO_OK) perr[(size_t)d] = hypo_gpu_last_error();
            };
            if (_n_ctx == 1) job(); else th.emplace_back(job);
        }
        for (auto& t : th) t.join();
        for (int d = 0; d < _n_ctx; ++d) n_resident += _device_arms[(size_t)d]->polished_windows();      // (windows a context owns: its halo's are another's)
        hypo_gpu_use_device(0);
        for (int d = 0; d < _n_ctx; ++d) {
            if (prc[(size_t)d] != HYPO_OK) { std::fprintf(stderr, "[Hypo::Window] Error: %s\n", perr[(size_t)d].c_str()); std::exit(1); }
            wins.insert(wins.end(), retry[(size_t)d].begin(), retry[(size_t)d].end());
        }
    }
    if (Window::generate_consensus_batch(wins) != HYPO_OK) { std::fprintf(stderr, "[Hypo::Window] Error: %s\n", hypo_gpu_last_error()); std::exit(1); }
    std::fprintf(stdout, "[Hypo::Hypo] Info: polished windows (Batch %u): %lu\n", b.batch_id, (unsigned long)(wins.size() + n_resident));
    stop("[Hypo:Hypo]: POA of windows. ");
}

void Hypo::dump_regions(const Batch& batch) {
    for (uint32_t i = batch.initial_cid; i < batch.final_cid; ++i)
        for (uint64_t w = 0; w < _contigs[i]->get_num_regions(); ++w) {
            uint32_t b, e; RegionType t;
            _contigs[i]->region((uint32_t)w, b, e, t);
            const Window* win = _contigs[i]->window((uint32_t)w);
            if (!win && t != RegionType::SR && t != RegionType::MSR && !_cFlags.lr_bam_filename.empty()) continue;   // swallowed by a LONG window
            if (win) e = b + (uint32_t)win->get_window_len();           // a LONG window spans the arm-less regions that follow it
            _dump << _contigs[i]->get_name() << '\t' << b << '\t' << e << '\t' << region_name(t);
            if (win) _dump << '\t' << win->dump_counts() << '\t' << win->arms_crc32() << '\t' << win->get_consensus();
            if (win && std::getenv("HYPO_REGION_DUMP_ARMS")) _dump << '\t' << (win->is_long() ? "L" : "S") << '\t' << win->dump_text();
            else if (t != RegionType::SR && t != RegionType::MSR) _dump << "\t0\t0\t0\t0\t0\t" << _contigs[i]->draft_segment(b, e);   // no arms: draft kept
            _dump << '\n';
        }
}

// the writer thread: one batch's contigs go to the FASTA (and the VCF, and the k-mer set's query) while the next batch is processed
void Hypo::write_batch(WriterJob job, Extras& ex, RunOutputs& out) {
    const uint32_t initial_cid = job.initial_cid, final_cid = job.final_cid;
    std::ofstream& ofile = out.fasta();
    std::ofstream& vfile = out.vcf();
    omp_set_num_threads(std::max(1, std::min((int)_cFlags.threads, 8)));
    std::unique_ptr<EditBatchResult> edits;
    if (ex.edit_fn || ex.guard_on) {
        edits.reset(new EditBatchResult());
        if (hypo_gpu_use_device(0) != HYPO_OK || edit_scripts_for(ex.guard_on ? ex.guard_edit_fn : ex.edit_fn, _contigs, initial_cid, final_cid, *edits) != HYPO_OK)
            writer_fatal("edit scripts");
    }
    // Every contig takes one path.  Its source: under --kmer-guard the batch's records are made first, their clusters judged by the
    // set, and the contig comes as its draft, the draft with the accepted records applied, and the records with the rejected ones
    // marked; otherwise as its draft and its polished text.  --kmer-fix: the text goes through the fixes, and what comes back takes
    // its place; --kmer-bridge: that text goes through the bridges, likewise.  Its sink: the FASTA record, and both texts to the reports (the set's queries on context 0, the marks).
    const char* stage = "k-mer set query";
    int rc = ex.text_on || ex.fix_on || ex.bridge_on ? hypo_gpu_use_device(0) : HYPO_OK;
    const KmerFix::Emit file_text = [&](uint32_t c, const std::string& draft, const std::string& text) {
        ofile << ">" << _contigs[c]->get_name() << std::endl << text << std::endl;      // (operator<<'s bytes)
        return ex.texts(c, draft, text);
    };
    // (what the fixes hand on: to the bridges when they are on, to the file otherwise)
    const KmerFix::Emit bridge_text = [&](uint32_t c, const std::string& draft, const std::string& text) {
        return ex.bridge.push(c, _contigs[c]->get_name(), draft, text, file_text);
    };
    const KmerFix::Emit& fixed_text = ex.bridge_on ? bridge_text : file_text;
    auto text_out = [&](uint32_t c, auto&& draft, auto&& text) {
        if (!ex.fix_on && !ex.bridge_on) return file_text(c, draft, text);
        std::string d = ex.text_on ? std::string(std::forward<decltype(draft)>(draft)) : std::string();
        if (!ex.fix_on) return ex.bridge.push(c, _contigs[c]->get_name(), std::move(d), std::forward<decltype(text)>(text), file_text);
        return ex.fix.push(c, _contigs[c]->get_name(), std::move(d), std::forward<decltype(text)>(text), fixed_text);
    };
    // the VCF records while the contig's windows exist, then the windows go; recs: the guard's, with which of them it rejected
    auto records_out = [&](uint32_t c, const VcfContigRecords* recs, const std::vector<uint8_t>* rejected) {
        if (recs && ex.edit_fn) vcf_write_records(vfile, *_contigs[c], *recs, rejected);
        if (!recs && edits) vcf_records(vfile, *_contigs[c], *edits, c - initial_cid, ex.vstats);
        _contigs[c]->release_after_output();
    };
    if (rc == HYPO_OK && ex.guard_on) {
        stage = "k-mer guard";
        VcfStats unused;
        rc = ex.guard.run_batch(_contigs, initial_cid, final_cid, *edits, ex.edit_fn ? ex.vstats : unused,
            [&](uint32_t c, const std::string& draft, const std::string& text, const VcfContigRecords& recs, const std::vector<uint8_t>& rejected) {
                records_out(c, &recs, &rejected);
                return text_out(c, draft, text);
            });
    } else if (ex.text_on || ex.fix_on || ex.bridge_on) {
        if (ex.fix_on) stage = "k-mer fix / k-mer set query";
        else if (ex.bridge_on) stage = "k-mer bridge / k-mer set query";
        for (uint32_t c = initial_cid; c < final_cid && rc == HYPO_OK; ++c) {
            std::string text = _contigs[c]->polished_text();
            std::string draft = ex.text_on ? _contigs[c]->draft_segment(0, (uint32_t)_contigs[c]->get_len()) : std::string();
            records_out(c, nullptr, nullptr);
            rc = text_out(c, std::move(draft), std::move(text));
        }
    } else {
        // the plain run: the record is streamed, no report wants its text
        for (uint32_t c = initial_cid; c < final_cid; ++c) { ofile << *_contigs[c]; records_out(c, nullptr, nullptr); }
    }
    if (rc == HYPO_OK && ex.fix_on) { stage = "k-mer fix / k-mer set query"; rc = ex.fix.flush(fixed_text); }
    if (rc == HYPO_OK && ex.bridge_on) { stage = "k-mer bridge / k-mer set query"; rc = ex.bridge.flush(file_text); }
    if (rc == HYPO_OK) { stage = "k-mer set query"; rc = ex.texts_flush(); }
    if (rc != HYPO_OK) writer_fatal(stage);
}

// ---- once per run, behind the batches ---------------------------------------------------------------------------------------
void Hypo::commit_outputs(Extras& ex, RunOutputs& out) {
    start();
    if (_writer.joinable()) _writer.join();
    // --qv-spectra: the two spectra leave the device before the set goes
    if (ex.spectra_on) {
        if (hypo_gpu_use_device(0) != HYPO_OK || ex.spectra.fetch(_cFlags.qv_reliable_min) != HYPO_OK) ex.set_fail("hypo_gpu_kset_spectrum");
        ex.spectra.write(out.open_spectra(_cFlags.qv_spectra_filename));
    }
    // --qv-cn: every contig's final text is marked (here, or by --qv-spectra above); the depth pass runs before the set goes
    if (ex.cn_on) {
        const char* what = "";
        const int rc = hypo_gpu_use_device(0) != HYPO_OK ? HYPO_E_HIP : ex.cn.run(what);
        if (rc == CnReport::E_NO_PEAK) {
            std::fprintf(stderr, "[Hypo::QV] Error: --qv-cn: the read k-mer histogram has no peak at or above its valley, so the read count of one copy is unknown: give it with --qv-cn-unit\n");
            ex.set.end();
            std::exit(1);
        }
        if (rc != HYPO_OK) ex.set_fail(what);
    }
    if (ex.fix_on) ex.fix.write(out.open_fixes(_cFlags.kmer_fix_filename));
    if (ex.bridge_on) ex.bridge.write(out.open_bridges(_cFlags.kmer_bridge_filename));
    // the set has answered its last query
    if (ex.set_on) ex.set.end();
    // --qv, --qv-bed: the table and the track are formatted once, closed and checked like the others
    if (ex.ask_on) {
        std::vector<std::string> names;
        for (const auto& c : _contigs) names.push_back(c->get_name());
        if (ex.qv_on) ex.qv.write(out.open_qv(_cFlags.qv_filename), names);
        if (ex.bed_on) ex.qv.write_track(out.open_bed(_cFlags.qv_bed_filename), names);
    }
    if (ex.cn_on) {
        std::vector<std::string> names;
        for (const auto& c : _contigs) names.push_back(c->get_name());
        ex.cn.write(out.open_cn(_cFlags.qv_cn_filename), names);
    }
    out.commit([&](RunOutputs::Which w) {
        if (w == RunOutputs::FASTA && ex.guard_on && ex.guard.by_record()) {
            const KmerGuard::Stats& gs = ex.guard.stats();
            std::fprintf(stdout, "[Hypo::Hypo] Info: k-mer guard (k = %u, by record in clusters of up to %u): %llu clusters of %llu records, %llu clusters rejected whole, %llu in part, %llu records rejected\n",
                         ex.guard.k(), ex.guard.max_records(), (unsigned long long)gs.clusters, (unsigned long long)gs.records, (unsigned long long)gs.rejected_clusters,
                         (unsigned long long)gs.partial_clusters, (unsigned long long)gs.rejected_records);
            if (std::getenv("HYPO_STAGE_COUNTERS")) {
                std::fprintf(stdout, "[Hypo::Hypo] Info: k-mer guard: clusters by number of records:");
                for (uint32_t n = 1; n <= ex.guard.max_records(); ++n) std::fprintf(stdout, " %u: %llu,", n, (unsigned long long)gs.by_size[n]);
                std::fprintf(stdout, " > %u: %llu\n", ex.guard.max_records(), (unsigned long long)gs.by_size[0]);
            }
        } else if (w == RunOutputs::FASTA && ex.guard_on)
            std::fprintf(stdout, "[Hypo::Hypo] Info: k-mer guard (k = %u): %llu clusters of %llu records, %llu clusters (%llu records) rejected\n", ex.guard.k(),
                         (unsigned long long)ex.guard.stats().clusters, (unsigned long long)ex.guard.stats().records, (unsigned long long)ex.guard.stats().rejected_clusters,
                         (unsigned long long)ex.guard.stats().rejected_records);
        if (w == RunOutputs::VCF)
            std::fprintf(stdout, "[Hypo::Hypo] Info: VCF %s: %llu records, %llu substituted, %llu inserted, %llu deleted bases\n", _cFlags.vcf_filename.c_str(),
                         (unsigned long long)ex.vstats.records, (unsigned long long)ex.vstats.sub, (unsigned long long)ex.vstats.ins, (unsigned long long)ex.vstats.del);
        if (w == RunOutputs::QV)
            std::fprintf(stdout, "[Hypo::Hypo] Info: QV %s (k = %u, %llu distinct read k-mers): draft %s, polished %s\n", _cFlags.qv_filename.c_str(), ex.set.k(),
                         (unsigned long long)ex.set.n_distinct(), ex.qv.draft_qv().c_str(), ex.qv.polished_qv().c_str());
        if (w == RunOutputs::SPECTRA)
            std::fprintf(stdout, "[Hypo::Hypo] Info: spectra %s (k = %u, reliable >= %u): completeness draft %s, polished %s\n", _cFlags.qv_spectra_filename.c_str(), ex.spectra.k(),
                         ex.spectra.threshold(), ex.spectra.completeness(SpectraReport::DRAFT).c_str(), ex.spectra.completeness(SpectraReport::POLISHED).c_str());
        if (w == RunOutputs::FIXES) {
            const KmerFix::Stats& fs = ex.fix.stats();
            std::fprintf(stdout, "[Hypo::Hypo] Info: k-mer fix %s (k = %u): %llu intervals, %llu sites, %llu fixed (%llu sub, %llu del, %llu ins), %llu ambiguous, %llu missing k-mers removed\n",
                         _cFlags.kmer_fix_filename.c_str(), ex.fix.k(), (unsigned long long)fs.intervals, (unsigned long long)fs.sites, (unsigned long long)fs.fixed,
                         (unsigned long long)fs.sub, (unsigned long long)fs.del, (unsigned long long)fs.ins, (unsigned long long)fs.ambiguous, (unsigned long long)fs.removed);
        }
        if (w == RunOutputs::BRIDGES) {
            const KmerBridge::Stats& bs = ex.bridge.stats();
            std::fprintf(stdout, "[Hypo::Hypo] Info: k-mer bridge %s (k = %u, max %u, slack %u): %llu intervals, %llu sites, %llu bridged (%llu bases out, %llu bases in), %llu ambiguous, "
                                 "%llu over budget, %llu missing k-mers removed\n", _cFlags.kmer_bridge_filename.c_str(), ex.bridge.k(), ex.bridge.max_dist(), ex.bridge.slack(),
                         (unsigned long long)bs.intervals, (unsigned long long)bs.sites, (unsigned long long)bs.bridged, (unsigned long long)bs.bases_out,
                         (unsigned long long)bs.bases_in, (unsigned long long)bs.ambiguous, (unsigned long long)bs.over_budget, (unsigned long long)bs.removed);
            if (ex.vote_on) {
                const KmerBridge::VoteStats& vs = ex.bridge.vote_stats();
                std::fprintf(stdout, "[Hypo::Hypo] Info: k-mer bridge vote (ratio %u, up to %u walks): %llu asked, %llu chosen, %llu too close, %llu more than %u walks, %llu over budget\n",
                             ex.bridge.vote_ratio(), (unsigned)HYPO_KSET_MAX_WALKS, (unsigned long long)vs.asked, (unsigned long long)vs.chosen, (unsigned long long)vs.close,
                             (unsigned long long)vs.many, (unsigned)HYPO_KSET_MAX_WALKS, (unsigned long long)vs.over_budget);
            }
        }
        if (w == RunOutputs::CN) {
            const CnReport::Sums cs = ex.cn.sums();
            std::fprintf(stdout, "[Hypo::Hypo] Info: copy number %s (k = %u, bin = %u, unit = %u %s): %llu bins, %llu collapsed (%llu bases), %llu duplicated (%llu bases)\n",
                         _cFlags.qv_cn_filename.c_str(), ex.cn.k(), ex.cn.bin(), ex.cn.unit(), ex.cn.unit_given() ? "given" : "peak", (unsigned long long)cs.bins,
                         (unsigned long long)cs.collapsed, (unsigned long long)cs.collapsed_bases, (unsigned long long)cs.duplicated, (unsigned long long)cs.duplicated_bases);
        }
        if (w == RunOutputs::BED) {
            const QvReport::TrackSums ts = ex.qv.track_sums();
            std::fprintf(stdout, "[Hypo::Hypo] Info: QV track %s (k = %u): %llu intervals covering %llu bases, %llu missing k-mers\n", _cFlags.qv_bed_filename.c_str(), ex.set.k(),
                         (unsigned long long)ts.intervals, (unsigned long long)ts.bases, (unsigned long long)ts.missing);
        }
    });
    stop("[Hypo:Hypo]: Writing results. ");
}

// ---- the flat path of the short reads (ReadBatch.hpp) -------------------------------------------------------------------------
void Hypo::materialize_alignments(Batch& b, uint32_t c0, uint32_t c1) {
    for (uint32_t c = c0; c < c1; ++c) {
        char& d = b.materialized[c - b.initial_cid];
        if (d) continue;
        d = 1;
        _reads.materialize(c, _alignment_store[c]);
    }
}

void Hypo::parse_block(const SamReader& sf, const SamReader::RecordBlock& raw, ParsedBlock& blk, bool long_reads) {
    const uint32_t mq = _cFlags.map_qual_th;
    const size_t count = raw.n();
    blk.n = count;
    blk.status.assign(count, ParsedBlock::ST_SKIPPED);
    blk.cid.assign(count, -1);
    blk.bad_ref_name.clear();
    // (a block of long reads is a few thousand records of 10+ kb: shares small enough for every thread to get some)
    const int T = (int)std::max<size_t>(1, std::min<size_t>((size_t)omp_get_max_threads(), count / (long_reads ? 8 : 512) + 1));
    blk.chunks.resize((size_t)T);
#pragma omp parallel num_threads(T)
    {
        SamRecord rec;                                   // one per thread: its strings and CIGAR vector are reused
        int32_t tid_seen = -2; int64_t cid_seen = -1;
        for (int c = omp_get_thread_num(); c < T; c += omp_get_num_threads()) {
            ReadChunk& ch = blk.chunks[(size_t)c];
            ch.clear();
            const size_t a = count * (size_t)c / (size_t)T, b = count * ((size_t)c + 1) / (size_t)T;
            const bool bam = sf.is_bam();
            for (size_t i = a; i < b; ++i) {
                SamReader::BamCore bc;
                const bool direct = bam && sf.bam_core(raw.rec(i), raw.len(i), bc);       // BAM: fixed fields in place, bases straight from 4 to 2 bits
                if (direct) {
                    if ((bc.flag & (SAM_FUNMAP | SAM_FSECONDARY | SAM_FQCFAIL | SAM_FDUP)) || bc.mapq < mq) continue;
                    rec.tid = bc.tid; rec.pos = bc.pos; rec.flag = bc.flag; rec.mapq = bc.mapq;
                    rec.cigar.resize(bc.n_cigar);
                    if (bc.n_cigar) std::memcpy(rec.cigar.data(), bc.cigar, 4ull * bc.n_cigar);
                    rec.qname.assign(bc.qname, bc.l_qname);
                    if (long_reads) rec.has_nm = sf.bam_nm(raw.rec(i), raw.len(i), bc, rec.nm);
                } else {
                    sf.parse(raw.rec(i), raw.len(i), rec);
                    if ((rec.flag & (SAM_FUNMAP | SAM_FSECONDARY | SAM_FQCFAIL | SAM_FDUP)) || rec.mapq < mq) continue;
                }
                if (rec.tid != tid_seen) {                 // (one look-up per run of records of a contig)
                    auto it = rec.tid < 0 ? _cname_to_id.end() : _cname_to_id.find(sf.tid2name(rec.tid));
                    tid_seen = rec.tid;
                    cid_seen = it == _cname_to_id.end() ? -1 : (int64_t)it->second;
                }
                if (cid_seen < 0) { blk.status[i] = ParsedBlock::ST_BADREF; continue; }
                blk.cid[i] = (int32_t)cid_seen;
                uint32_t rb, re, qab, qae;
                Alignment::span_of(*_contigs[(size_t)cid_seen], rec, rb, re, qab, qae);
                const uint32_t qlen = qae - qab;
                // a long read is dropped when its NM-based normalised edit distance exceeds the threshold; the reference divides the
                // integers first (edit_dist * 100 / rlen) and compares the quotient (Alignment.cpp:51-58)
                if (long_reads && rec.has_nm && re > rb && (double)(rec.nm * 100 / (int64_t)(re - rb)) > (double)_cFlags.norm_edit_th) { blk.status[i] = ParsedBlock::ST_INVALID; continue; }
                // Alignment.cpp:551-571: the aligned part 2-bit packed; a read with a non-ACGT base there is dropped
                bool ok = (size_t)qab + qlen <= (direct ? (size_t)bc.l_seq : rec.seq.size());
                const size_t at = ch.seq.size();
                if (ok) {
                    ch.seq.resize(at + (qlen + 3) / 4);
                    ok = direct ? pack2_from_bam4(bc.seq4, qab, qlen, ch.seq.data() + at) : pack2_acgt(rec.seq.data() + qab, qlen, ch.seq.data() + at);
                    if (!ok) ch.seq.resize(at);
                }
                if (!ok) { blk.status[i] = ParsedBlock::ST_INVALID; continue; }
                blk.status[i] = ParsedBlock::ST_KEPT;
                ch.raw.push_back((uint32_t)i); ch.cid.push_back((int32_t)cid_seen); ch.rb.push_back(rb); ch.re.push_back(re); ch.qae.push_back(qlen);
                ch.cig.insert(ch.cig.end(), rec.cigar.begin(), rec.cigar.end());
                ch.seq_at.push_back((uint32_t)ch.seq.size()); ch.cig_at.push_back((uint32_t)ch.cig.size());
            }
        }
    }
    for (size_t i = 0; i < count; ++i)
        if (blk.status[i] == ParsedBlock::ST_BADREF) { blk.bad_ref_name = sf.record_name(raw.rec(i), raw.len(i)); break; }
}

// src/Hypo.cpp:278-329 for the short reads: stream the (coordinate-sorted) file, stop when a record of the next batch shows up.
// A reader thread inflates the file and cuts the next block of raw records while this block is parsed on all threads, every
// thread writing the records of its stretch into a chunk of flat arrays; the batch takes the kept records as slices of the block.
void Hypo::create_alignments_flat(uint32_t batch_id, ReadBatch& into, bool is_sr) {
    SamReader& sf = is_sr ? *_sf_short : *_sf_long;
    RecordStream& rs = is_sr ? _rs_short : _rs_long;
    const uint32_t final_cid = batch_id * _contig_batch_size + _contig_batch_size;
    uint64_t num_invalid = 0, num_alns = 0;
    constexpr size_t kBlock = 1 << 19, kBlockBytes = (size_t)128 << 20;     // (a block of records = about one run of inflated BGZF blocks, SeqIO.hpp)
    // (the record a call consumed for a contig behind its batch: a short read opens that contig's batch; a LONG read has been filed
    // as an object in that contig's store entry by Hypo::polish, where the reference's short-read phases find it)
    rs.opened_with_cid = -1;
    if (rs.carry_blk && is_sr) { into.add(rs.carry_blk, rs.carry_r0, rs.carry_r1); rs.opened_with_cid = rs.carry_cid; }
    rs.carry_blk.reset();
    bool stop = false, more_ahead = true;
    double t_wait = 0, t_par = 0, t_col = 0; auto now = []{ return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    if (!rs.reader) { rs.reader.reset(new BlockReader()); rs.reader->start(&sf); }
    while (!stop) {
        bool asked = false;
        const double t0 = now();
        if (!rs.parsed || rs.ppos >= rs.parsed->n) {
            if (rs.have_ahead) { std::swap(rs.cur, rs.ahead); rs.have_ahead = false; }
            else if (rs.more) rs.more = sf.read_block(rs.cur, kBlock, kBlockBytes);
            else break;
            if (rs.cur.n() == 0) { if (!rs.more) break; continue; }
            if (rs.more && !rs.have_ahead) { rs.reader->request(&rs.ahead, kBlock, kBlockBytes); asked = true; }
            std::shared_ptr<ParsedBlock> blk;
            {
                std::lock_guard<std::mutex> lk(_pool_mu);
                if (rs.parsed && rs.parsed.use_count() == 1 && _block_pool.size() < 8) _block_pool.push_back(std::move(rs.parsed));
                rs.parsed.reset();
                if (!_block_pool.empty()) { blk = std::move(_block_pool.back()); _block_pool.pop_back(); }
            }
            if (!blk) blk = std::make_shared<ParsedBlock>();
            const double t1 = now(); t_wait += t1 - t0;
            parse_block(sf, rs.cur, *blk, !is_sr);
            t_par += now() - t1;
            rs.parsed = blk; rs.ppos = 0;
        }
        const double t2 = now();
        const ParsedBlock& B = *rs.parsed;
        // where the batch ends: the first record that is not skipped and belongs to a contig of a later batch is consumed as well,
        // as in the reference; a record with an unknown reference before that is fatal
        size_t s_first = B.n;
        for (size_t i = rs.ppos; i < B.n; ++i) {
            const uint8_t st = B.status[i];
            if (st == ParsedBlock::ST_SKIPPED) continue;
            if (st == ParsedBlock::ST_BADREF) {
                std::fprintf(stderr, "[Hypo::Hypo] Error: Alignment File error: Contig-reference of record %s does not exist in the draft!\n", B.bad_ref_name.c_str());
                // (this may be the helper thread, with the main thread inside a device call: leave without running the static
                // destructors under it)
                std::fflush(nullptr);
                RunOutputs::discard();
                std::_Exit(1);
            }
            if (st == ParsedBlock::ST_KEPT) ++num_alns; else ++num_invalid;
            if ((uint32_t)B.cid[i] >= final_cid) { s_first = i; break; }
        }
        into.add(rs.parsed, rs.ppos, s_first);
        if (s_first < B.n) {
            if (B.status[s_first] == ParsedBlock::ST_KEPT) { rs.carry_blk = rs.parsed; rs.carry_r0 = s_first; rs.carry_r1 = s_first + 1; rs.carry_cid = B.cid[s_first]; }
            rs.ppos = s_first + 1;
            stop = true;
        } else rs.ppos = B.n;
        const double t3 = now();
        t_col += t3 - t2;
        if (asked) { more_ahead = rs.reader->wait(); rs.more = more_ahead; rs.have_ahead = rs.ahead.n() > 0; }
        t_wait += now() - t3;
    }
    if (std::getenv("HYPO_HOST_TIMING")) std::fprintf(stderr, "[timing] create_alignments_flat: waiting for records %.3f s, parse %.3f s, into the batch %.3f s (BGZF blocks: %s)\n", t_wait, t_par, t_col, BlockInflater::name());
    std::fprintf(stdout, "[Hypo::Hypo] Info: Number of alignments (Batch %u): loaded (%lu) invalid (%lu)\n", batch_id,
                 (unsigned long)num_alns, (unsigned long)num_invalid);
}

}  // namespace hypo
