// kset_kernel.hpp — host-visible interface of kset_kernel.hip (internal to libhypo_gpu.so): an exact set of canonical k-mers
// (k = 12..31) as an open-addressing hash table in HBM, filled from read bytes and queried with contig text (hypo --qv;
// DESIGN.md "k-mer QV").
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hypo {

constexpr uint64_t KSET_EMPTY = ~0ull;             // a key has 2k <= 62 bits: all-ones never is one
// The host keeps count <= KSET_MAX_LOAD * slots between calls (linear probing: ~1.5 probes for a key that is there, ~2.5 for one
// that is not, at one half).
constexpr double KSET_MAX_LOAD = 0.5;
constexpr uint64_t KSET_MIN_SLOTS = 1024;
constexpr int KS_THREADS = 256;                    // lanes of a workgroup, in every kernel of kset_kernel.hip

// Counters of a table (device memory): [0] keys in the table, [1] overflow flag (a lane found no room within `slots` probes).
// table: `slots` 64-bit words, KSET_EMPTY where free (a fresh table is filled with 0xff bytes).  All pointers are device pointers.
// every canonical k-mer of bytes[0, n) (the byte rules of kmer_count_run) into the table; ctr[0] += new keys
hipError_t kset_insert_run(const uint8_t* bytes, uint64_t n, uint32_t k, uint64_t* table, uint64_t slots, unsigned long long* ctr, hipStream_t st);
// every key of `old_table` into `table` (which must not hold any of them yet); ctr[0] += keys moved
hipError_t kset_rehash_run(const uint64_t* old_table, uint64_t old_slots, uint64_t* table, uint64_t slots, unsigned long long* ctr, hipStream_t st);
// Read counts and copy numbers (hypo --qv-spectra; DESIGN.md "k-mer spectra").  planes: (1 + n_texts) * ks_plane_words(slots) 32-bit
// words beside a table of `slots` slots, zero when fresh; byte s of plane 0 is the count of the key in slot s (the windows of the
// reads, stopping at 255), byte s of plane 1 + t the windows of text t (likewise).  A plane is padded to whole 256-slot blocks.
constexpr uint32_t KSET_MAX_TEXTS = 4;
constexpr uint32_t KSET_HIST_COLS = 5, KSET_HIST_BINS = 256 * KSET_HIST_COLS;      // hist[count * 5 + min(copy number, 4)]
uint64_t ks_plane_words(uint64_t slots);
// kset_insert_run, and every window adds one to its key's count byte: a window handed in twice is counted twice
hipError_t kset_insert_count_run(const uint8_t* bytes, uint64_t n, uint32_t k, uint64_t* table, uint64_t slots, unsigned long long* ctr,
                                 uint32_t* planes, hipStream_t st);
// kset_rehash_run, and every key's count byte goes with it (the copy bytes must still be zero: they stay behind)
hipError_t kset_rehash_count_run(const uint64_t* old_table, uint64_t old_slots, const uint32_t* old_planes, uint64_t* table, uint64_t slots,
                                 uint32_t* planes, unsigned long long* ctr, hipStream_t st);
// the sequences of kset_query_run: a window whose key is in the table adds one to the key's byte of text `text`; sums[0] += all
// windows, sums[1] += those whose key is not in the table (zeroed by the caller)
hipError_t kset_mark_run(const uint8_t* bytes, const uint64_t* off, uint32_t n_seqs, uint64_t n, uint32_t k, const uint64_t* table, uint64_t slots,
                         uint32_t* planes, uint32_t text, unsigned long long* sums, hipStream_t st);
// hist[c * 5 + j] += the keys with count byte c and min(copy byte of `text`, 4) == j; KSET_HIST_BINS values, zeroed by the caller
hipError_t kset_spectrum_run(const uint32_t* planes, uint64_t slots, uint32_t text, unsigned long long* hist, hipStream_t st);
// What a query reads of the set: the table of `slots` slots, k, and the least count (hypo --qv-min-count; DESIGN.md "k-mer min
// count").  The launchers below that take one get the planes of a set that counts and min_count = t: with t >= 2 they answer against
// R_t, the keys whose count byte is at least t, with kernels of their own (kset_*_min_kernel); with t <= 1 they launch the kernels
// they always launched and `planes` is not looked at (it may be NULL).
struct KsetView { const uint64_t* table; uint64_t slots; uint32_t k; const uint32_t* planes; uint32_t min_count; };
// n_seqs byte strings back to back in bytes[0, off[n_seqs]) (off[0] = 0): total[s] += length-k windows of sequence s made of
// ACGTacgt only, missing[s] += those whose canonical k-mer is not in the table.  total / missing must be zeroed by the caller.
hipError_t kset_query_run(const KsetView& set, const uint8_t* bytes, const uint64_t* off, uint32_t n_seqs, uint64_t n, unsigned long long* total,
                          unsigned long long* missing, hipStream_t st);
// The same query, and where the missing windows are (hypo --qv-bed; DESIGN.md "k-mer QV track"), in two steps with the caller
// reading pre[3 blocks .. 3 blocks + 3) = (intervals, intervals, missing windows of wanted sequences) in between, blocks =
// kset_track_blocks(n).  want: NULL or n_seqs bytes, 0 = no intervals for that sequence.  Work space: miss_bits / begin_bits of
// KS_THREADS * blocks words each, sums of blocks and pre of 3 * (blocks + 1) 64-bit words; none needs clearing.
//   count: total / missing as kset_query_run (zeroed by the caller), the flag words, their per-workgroup sums and the prefixes.
//   emit:  iv_off[n_seqs + 1], and n_iv intervals in ascending order: iv_start / iv_end relative to the interval's sequence,
//          cnt_hi = its missing windows (cnt_lo is work space).  Every array has n_iv entries; n_iv must be the total read from pre.
uint32_t kset_track_blocks(uint64_t n);
hipError_t kset_track_count_run(const KsetView& set, const uint8_t* bytes, const uint64_t* off, uint32_t n_seqs, uint64_t n, unsigned long long* total,
                                unsigned long long* missing, const uint8_t* want, uint32_t* miss_bits, uint32_t* begin_bits, uint64_t* sums, uint64_t* pre,
                                hipStream_t st);
hipError_t kset_track_emit_run(const uint64_t* off, uint32_t n_seqs, uint64_t n, uint32_t k, const uint32_t* miss_bits, const uint32_t* begin_bits,
                               const uint64_t* pre, uint64_t n_iv, uint64_t* iv_off, uint64_t* iv_start, uint64_t* iv_end, uint64_t* cnt_lo,
                               uint64_t* cnt_hi, hipStream_t st);
// n_items pieces of spans: item i is bytes[item_lo[i], item_lo[i] + item_len[i]), no window crosses its ends; out[i] = (its windows
// made of ACGTacgt only, those not in the table).  A group of `group` lanes (32 or 64) owns an item; the caller cuts a span into
// items of at most KSET_SPAN_PIECE windows (consecutive items overlap by k - 1 bytes) and adds their results up.
constexpr uint32_t KSET_SPAN_PIECE = 2048;
constexpr int KSET_SPAN_GROUP = 32;                // the default geometry (DESIGN.md "k-mer guard": measured against 64)
hipError_t kset_spans_run(const KsetView& set, const uint8_t* bytes, const uint64_t* item_lo, const uint32_t* item_len, uint32_t n_items, uint2* out,
                          int group, hipStream_t st);

// Every subset of the edits of n_sites sites (hypo --guard-records).  The caller has checked every range (see the bounds comment of
// the kernels).
constexpr uint32_t KSET_MAX_EDITS = 12;
struct KsetVariantsIn {
    const uint8_t *bytes, *alts;                       // the text and the ALT bytes
    const uint64_t* site_lo;                           // site s is bytes[site_lo[s], ..)
    const uint32_t* edit_off;                          // with the edits [edit_off[s], edit_off[s + 1]): at most KSET_MAX_EDITS, ascending and disjoint
    const uint64_t *eb, *ee, *ao; const uint32_t* al;  // edit e replaces bytes[eb[e], ee[e]) by alts[ao[e], ao[e] + al[e]); variant `mask` of a site takes the ALT of its edit j when bit j is set
    // (site, mask, first byte of the piece in the variant's text, bytes of the piece), in site order, within a site in mask order,
    // within a variant in text order, every variant with at least one item (w = 0: no window)
    const uint4* items; uint32_t n_items;
    const uint32_t* site_item;                         // site_item[s] = the first item of site s (n_sites + 1 entries)
    const uint32_t* var_off;                           // var_off[s] = the variants of the sites before s
    uint32_t n_sites;
};
struct KsetVariantsOut {
    uint2* item_res;                                   // n_items pairs of work space
    uint32_t* best_mask; unsigned long long *best_total, *best_missing;   // [s]: the variant with the fewest missing windows, then the most edits taken, then the greatest mask
    unsigned long long *var_total, *var_missing;       // (both or neither): every variant's pair at var_off[s] + mask
};
hipError_t kset_variants_run(const KsetView& set, const KsetVariantsIn& in, const KsetVariantsOut& out, int group, hipStream_t st);

// Every one-base edit of n_sites short regions (hypo --kmer-fix; DESIGN.md "k-mer fix").  A site's 9 w - 3 candidates, in this order:
// the span as it is; sub(p, b), p ascending over the region, b in ACGT order; del(p), p ascending; ins(p, b), b put in front of p, p
// ascending from the region's second byte.  The caller has checked every range (see the bounds comment of the kernels).
constexpr uint32_t KSET_MAX_FIX_REGION = 31;
constexpr uint32_t KSET_MAX_FIX_SPAN = 2048;
struct KsetFixesIn {
    const uint8_t* bytes;
    const uint64_t* site_lo; const uint32_t* site_len; // site s is the span bytes[site_lo[s], site_lo[s] + site_len[s])
    const uint32_t *site_c0, *site_w;                  // with the region of site_w[s] bytes that starts site_c0[s] bytes into it
    const uint32_t* item_off;                          // item_off[s] = the candidates of the sites before s (n_sites + 1 entries, n_items = item_off[n_sites])
    uint32_t n_sites, n_items;
};
struct KsetFixesOut {
    uint2* item_res;                                   // n_items pairs of work space
    unsigned long long *none_total, *none_missing;     // the unedited span's pair
    uint32_t* best_cand; unsigned long long *best_total, *best_missing;   // the canonical candidate (see the reduce kernel) with the fewest missing windows, the first among equals
    uint32_t* zeros;                                   // the canonical candidates with none missing
    unsigned long long *cand_total, *cand_missing;     // (both or neither): every candidate's pair at item_off[s] + j
};
hipError_t kset_fixes_run(const KsetView& set, const KsetFixesIn& in, const KsetFixesOut& out, int group, hipStream_t st);

// Walks through the set as a de Bruijn graph (hypo --kmer-bridge; DESIGN.md "k-mer bridge"): site s starts at the k-mer
// bytes[from[s], from[s] + k) and asks for the walks that arrive at bytes[to[s], to[s] + k) after dlo[s] .. dhi[s] steps, by the
// depth-first search of include/hypo_gpu.h with at most `budget` visits.  The caller has checked every range (see the bounds comment
// of the kernels): from + k and to + k inside the text, 1 <= dlo <= dhi <= KSET_MAX_WALK, 1 <= budget <= KSET_MAX_WALK_BUDGET.
constexpr uint32_t KSET_MAX_WALK = 256;
constexpr uint32_t KSET_MAX_WALK_BUDGET = 65536;
struct KsetWalkSites { const uint8_t* bytes; const uint64_t *from, *to; const uint32_t *dlo, *dhi; uint32_t n_sites; };
// status / steps / len: n_sites values each; walk: n_sites * KSET_MAX_WALK bytes, the first walk's bases at walk[s * KSET_MAX_WALK, + len[s]).
hipError_t kset_walks_run(const KsetView& set, const KsetWalkSites& sites, uint32_t budget, uint32_t* status, uint32_t* steps, uint32_t* len, uint8_t* walk,
                          hipStream_t st);
// The same search carried on to the first KSET_WALK_SETS walks, each with its support (hypo --kmer-bridge-vote; DESIGN.md "k-mer bridge
// vote"), on a set that counts: `planes` must not be NULL, a child exists iff its count byte is at least max(min_count, 1).  status
// / steps / n_walks: n_sites values each; len / low: n_sites * KSET_WALK_SETS, walk: n_sites * KSET_WALK_SETS * KSET_MAX_WALK bytes;
// walk w of site s sits at index s * KSET_WALK_SETS + w, in the order of arrival, low = the least count byte along it.  Slots at
// or beyond n_walks[s] are work space (under BUDGET they hold the walks found before it), as are the bytes beyond a walk's len: the
// caller passes on what lies below them only.  The caller has checked the ranges kset_walks_run asks for.
constexpr uint32_t KSET_WALK_SETS = 4;
hipError_t kset_walk_sets_run(const KsetView& set, const KsetWalkSites& sites, uint32_t budget, uint32_t* status, uint32_t* steps, uint32_t* n_walks,
                              uint32_t* len, uint32_t* low, uint8_t* walk, hipStream_t st);

// The set's records out and in (hypo --qv-save / --qv-load; DESIGN.md "k-mer set file").  A record: a key of the table and its count
// byte (1 when `planes` is NULL); its digest: mix64(key) + count * 0x9e3779b97f4a7c15.
// export: the keys of slots [s0, s0 + n_slots) (s0 + n_slots <= slots, n_slots <= cap) in ascending slot order into out_keys /
// out_counts (may be NULL), *digest += the sum of their digests, pre[tiles] = their number, tiles = kset_export_tiles(n_slots).
// Work space: sums of tiles and pre of tiles + 1 64-bit words; neither needs clearing.
uint32_t kset_export_tiles(uint64_t n_slots);
hipError_t kset_export_run(const uint64_t* table, const uint32_t* planes, uint64_t s0, uint64_t n_slots, uint64_t* sums, uint64_t* pre, uint64_t cap,
                           uint64_t* out_keys, uint8_t* out_counts, unsigned long long* digest, hipStream_t st);
// import, first the check: bad[0] = 1 and bad[1] = the least index i with keys[i] >= 4^k, keys[i] above its reverse complement, or
// counts[i] == 0 (counts may be NULL); the caller sets bad[] = {0, all-ones}.  Then the records into the table: ctr[0] += new keys,
// ctr[1] the overflow flag, with `planes` every key's count byte becomes min(255, byte + counts[i]) (NULL counts: 1 each), *digest
// += the sum of the records' digests.  The caller has made room for n new keys.
hipError_t kset_import_check_run(const uint64_t* keys, const uint8_t* counts, uint64_t n, uint32_t k, unsigned long long* bad, hipStream_t st);
hipError_t kset_import_run(const uint64_t* keys, const uint8_t* counts, uint64_t n, uint64_t* table, uint64_t slots, unsigned long long* ctr,
                           uint32_t* planes, unsigned long long* digest, hipStream_t st);

// Read count against copy number per bin of a text (hypo --qv-cn; DESIGN.md "k-mer copy number"), on a set that counts (`planes` must
// not be NULL).  The sequences are those of kset_query_run; sequence s has ceil(len / bin) bins, bin j of it owns the windows that
// start in [j bin, (j + 1) bin), and bin_off[s] = the bins of the sequences before s (n_seqs + 1 entries, bin_off[n_seqs] = n_bins).
// With c the window's count byte, m its copy byte of plane `text` and t = max(min_count, 1), per bin: windows; missing (not in the
// table, or c < t); rated (present, 1 <= m <= 254, c <= 254); over (rated, 2 c >= 3 unit m); under (rated, 4 c <= 3 unit m);
// med_count (the lower median of c over the present windows, 0 without one).  Every entry below n_bins is written; nothing needs
// clearing.  The caller has checked bin in KSET_DEPTH_MIN_BIN .. KSET_DEPTH_MAX_BIN, unit in 1..255 and bin_off.
constexpr uint32_t KSET_DEPTH_MIN_BIN = 32, KSET_DEPTH_MAX_BIN = 65536;
struct KsetDepthOut { uint32_t *windows, *missing, *rated, *over, *under; uint8_t* med_count; };
hipError_t kset_depth_run(const KsetView& set, const uint8_t* bytes, const uint64_t* off, const uint64_t* bin_off, uint32_t n_seqs, uint64_t n_bins,
                          uint32_t bin, uint32_t text, uint32_t unit, const KsetDepthOut& out, hipStream_t st);

}  // namespace hypo
