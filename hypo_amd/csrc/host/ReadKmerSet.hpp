// ReadKmerSet.hpp — the exact set of the canonical k-mers of the short reads on device context 0 (hypo_gpu_kset_*, kset_kernel.hip;
// DESIGN.md "k-mer QV"), from hypo_gpu_kset_begin to hypo_gpu_kset_end.  The parse pass of stage 0 fills it through sink(); then
// --qv and --qv-bed (QvReport), --qv-spectra (SpectraReport), --kmer-guard (KmerGuard) and --kmer-fix (KmerFix) ask it, each with
// an entry point of its own, bound where it is used.  What more than one of them needs is here: the set's k, its counts and the
// least count of --qv-min-count (DESIGN.md "k-mer min count"), the shape of the count histogram, the track query with its retry,
// and the bound on the text of one call.  --qv-cn (CnReport; DESIGN.md "k-mer copy number") asks through query_depth, which cuts
// the text into calls here.
#pragma once
#include <cstdint>
#include <string>
#include <vector>
#include "SolidBuild.hpp"

namespace hypo {

class ReadKmerSet {
public:
    static constexpr size_t kTextPerCall = (size_t)512 << 20;       // text per query, mark, spans or track call (a batch of small contigs: one call)
    static constexpr uint32_t kRows = 256, kCols = 5;            // hypo_gpu_kset_spectrum: hist[c * 5 + min(copy number, 4)], c = 0..255
    static constexpr const char* kNames = "hypo_gpu_kset_begin / _add / _size / _end";
    // the valley of a read histogram h[0 .. kRows): the smallest c in 2..254 at which it stops falling, h[c] <= h[c + 1]; 2 when it
    // never does (the default of --qv-reliable-min, and `valley` of --qv-min-count)
    static uint32_t valley(const uint64_t* h);

    // The entry points, bound by name: only runs that build the set need them.  bind: the four of kNames; bind_counts:
    // hypo_gpu_kset_counts_enable, _spectrum and _min_count; bind_track: hypo_gpu_kset_query_track.  false: the device library
    // lacks one of them, and the have_* say which group.
    bool bind();
    bool bind_counts();
    bool bind_track();
    bool have_set() const { return _begin && _add && _size && _end; }
    bool have_counts() const { return _counts_enable && _spectrum; }             // what --qv-spectra needs of the three
    bool have_min_count() const { return _set_min_count != nullptr; }
    bool have_track() const { return _track != nullptr; }
    // --qv-save / --qv-load: hypo_gpu_kset_export / hypo_gpu_kset_import
    bool bind_export();
    bool bind_import();

    // the set on the calling thread's context; max_bytes 0 = the library's default cap
    int begin(uint32_t k, uint64_t expected_distinct, uint64_t max_bytes);
    // once, right after begin: the set counts, and keeps n_texts planes of copy bytes (--qv-spectra: 2, --qv-min-count alone: 1)
    int enable_counts(uint32_t n_texts);
    ReadSink sink();                                         // (holds a pointer to the set; the caller sets `exact`)
    int reads_done();                                        // after the reads: fetches the number of distinct k-mers
    // --qv-min-count, after the reads and before the first query: reads the histogram of the read counts, takes t = `given` or, for
    // 0, its valley, and from then on every query of the set is answered against the k-mers seen at least t times
    int set_min_count(uint32_t given);
    // --qv-save / --qv-load: one call of hypo_gpu_kset_export / hypo_gpu_kset_import (host/KmerSetFile.hpp moves the records between
    // these and the file)
    int export_records(uint64_t* cursor, uint64_t* keys, uint8_t* counts, uint64_t cap, uint64_t* n_out, uint64_t* digest) const {
        return _export(cursor, keys, counts, cap, n_out, digest);
    }
    int import_records(const uint64_t* keys, const uint8_t* counts, uint64_t n, uint64_t* digest) { return _import(keys, counts, n, digest); }
    void end();                                              // frees the set (safe to call twice, and after a begin that failed)

    bool open() const { return _open; }
    uint32_t k() const { return _k; }
    uint64_t n_distinct() const { return _n_distinct; }
    uint32_t min_count() const { return _min_count; }
    uint64_t n_reliable() const { return _n_reliable; }      // distinct read k-mers seen at least min_count() times

    // hypo_gpu_kset_spectrum of one text plane: kRows * kCols values
    int spectrum(uint32_t text, std::vector<uint64_t>& hist) const;
    // hypo_gpu_kset_query_track over the sequences text[off[s], off[s + 1]), s < off.size() - 1 (want: per sequence, or NULL for all).
    // The first call has room for 1024 intervals and one per KiB of text; a call that finds more says how many, and a second call
    // with that room asks the set everything again (rare at one interval per kbp).  HYPO_OK or the C-ABI's error.
    struct Track { std::vector<uint64_t> total, missing, iv_off, start, end, count; };
    int query_track(const std::string& text, const std::vector<uint64_t>& off, const uint8_t* want, Track& out) const;

    // --qv-cn: hypo_gpu_kset_query_depth, bound by name (false: the device library lacks it)
    bool bind_depth();
    bool have_depth() const { return _depth != nullptr; }
    // the default unit of --qv-cn, of a read histogram h[0 .. kRows): the c in [valley(h), 254] with the largest h[c], the smallest such
    // c among equals; 0 when every h[c] in that range is 0
    static uint32_t peak(const uint64_t* h);
    // hypo_gpu_kset_query_depth over the sequences text[off[s], off[s + 1]) in bins of `bin` window starts against plane `plane`, a
    // copy worth `unit` reads: the six arrays of all bins, sequence by sequence.  The text goes in calls of at most per_call bytes
    // cut at sequence ends; a single longer sequence is cut at multiples of `bin`, each piece with the k - 1 bytes its last windows
    // need (the bin those bytes alone would open holds no window and is dropped), so the pieces' arrays concatenate to the answer of
    // one call.  HYPO_OK or the C-ABI's error.
    struct Depth { std::vector<uint32_t> windows, missing, rated, over, under; std::vector<uint8_t> median; };
    int query_depth(const std::string& text, const std::vector<uint64_t>& off, uint32_t bin, uint32_t plane, uint32_t unit, Depth& out,
                    size_t per_call = kTextPerCall) const;
private:
    int (*_depth)(const char*, const uint64_t*, uint32_t, uint32_t, uint32_t, uint32_t, uint64_t, uint32_t*, uint32_t*, uint32_t*, uint32_t*, uint32_t*, uint8_t*) = nullptr;
    int (*_begin)(uint32_t, uint64_t, uint64_t) = nullptr;
    int (*_add)(const char*, uint64_t) = nullptr;
    int (*_size)(uint64_t*, uint64_t*) = nullptr;
    int (*_end)(void) = nullptr;
    int (*_counts_enable)(uint32_t) = nullptr;
    int (*_spectrum)(uint32_t, uint64_t*) = nullptr;
    int (*_set_min_count)(uint32_t) = nullptr;
    int (*_track)(const char*, const uint64_t*, uint32_t, const uint8_t*, uint64_t*, uint64_t*, uint64_t*, uint64_t*, uint64_t*, uint64_t*, uint64_t) = nullptr;
    int (*_export)(uint64_t*, uint64_t*, uint8_t*, uint64_t, uint64_t*, uint64_t*) = nullptr;
    int (*_import)(const uint64_t*, const uint8_t*, uint64_t, uint64_t*) = nullptr;
    bool _open = false;
    uint32_t _k = 0, _min_count = 1;
    uint64_t _n_distinct = 0, _n_reliable = 0;
};

}  // namespace hypo
