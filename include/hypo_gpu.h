/*
 * hypo_gpu.h — C-ABI of the MI355X (gfx950) polishing hot path.
 *
 * The reference (kensung-lab/hypo) has no FFI: its hot path is reached through three C++ call
 * sites in Hypo::polish() (src/Hypo.cpp:100-103 solid scan, :237 prepare_for_poa, :238-247
 * per-window POA; results read at src/Contig.cpp:357).  This header is the boundary a maintainer
 * would bind there instead (see INTEGRATION.md for the C++ stub): plain pointers and sizes,
 * no C++ or torch types.  Every entry point cites the reference interface it replaces.
 *
 * Conventions
 *  - every function returns 0 on success, <0 = HYPO_E_* (never throws, never exits);
 *    hypo_gpu_last_error() gives a thread-local message.
 *  - "_device" variants take DEVICE pointers inside the batch structs and run asynchronously on the
 *    given hipStream_t (passed as void*; NULL = the HIP null stream, ordered after everything the caller queued there);
 *    plain variants take HOST pointers and do H2D/D2H themselves on a stream of the context.
 *    (hypo_gpu_poa_batch_device returns once all kernels are queued.  Only the first call of a context waits, for its own
 *    plan step; later calls size their launches from the plan of the call before them.)
 *  - one device context per device handed to hypo_gpu_init.  A host thread works on the context it selected with
 *    hypo_gpu_use_device (slot 0 until then); calls on different contexts run concurrently, the host part of calls on
 *    the same context (enqueueing, the copies of the host-buffer variants) is serialised inside the library.
 *  - sequences are packed exactly like the reference's PackedSeq<NB> (src/PackedSeq.cpp:58-89):
 *    MSB-first inside a byte, 2 bases/byte for NB=4 (codes A0 C1 G2 T3 N4), 4 bases/byte for NB=2.
 *    Every sequence starts on a byte boundary of its buffer.
 */
#ifndef HYPO_GPU_H
#define HYPO_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HYPO_GPU_ABI_VERSION 11
#define HYPO_MAX_DEVICES 16      /* contexts one process can hold (an MI355X node has 8 GPUs) */

/* error codes */
#define HYPO_OK              0
#define HYPO_E_INVALID      -1   /* bad argument (NULL pointer, k out of range, positive gap score ...) */
#define HYPO_E_NODEVICE     -2   /* no gfx950 device / hip runtime failure at init */
#define HYPO_E_HIP          -3   /* a HIP call failed (message in hypo_gpu_last_error) */
#define HYPO_E_WORKSPACE    -4   /* caller-provided workspace too small */
#define HYPO_E_NOTINIT      -5
#define HYPO_E_CAPACITY     -6   /* more than the 32-bit counters of the boundary hold: split the work; the k-mer set reached its cap */
#define HYPO_E_UNSUPPORTED  -7   /* this build of the library does not provide the entry point (test shims) */

/* per-window status byte written by the POA entry points */
#define HYPO_ST_OK            0
#define HYPO_ST_CONS_OVERFLOW 1  /* consensus longer than the caller's slot (len holds the needed size) */
#define HYPO_ST_CAPACITY      2  /* window exceeds the largest device size class */
#define HYPO_ST_UNDEFINED     3  /* input hits behaviour that is undefined in the reference
                                    (graph.cpp:184-200: alignment without any sequence position) */
#define HYPO_ST_INVALID       4  /* the window's descriptor points outside the batch's buffers (first_arm + arms > n_arms,
                                    draft_off / arm_off + bytes beyond draft4_bytes / arms2_bytes); nothing was read there */
#define HYPO_ST_UNWRITTEN  0xff  /* what every status byte holds when the kernels start (len = 0): a window that comes back with it
                                    was answered by no kernel - an internal error of the library, never a property of the window */

/* Reference: ScoreParams, include/globalDefs.hpp:58-66 (same field order, INT8 each). */
typedef struct HypoScoreParams {
    int8_t sr_match, sr_mismatch, sr_gap;
    int8_t lr_match, lr_mismatch, lr_gap;
} HypoScoreParams;

/* Reference: enum class WindowType, include/Window.hpp:35-38. */
#define HYPO_WIN_SHORT 0
#define HYPO_WIN_LONG  1

/*
 * One Window object, flattened.  Reference: data members of hypo::Window (include/Window.hpp:123-135).
 * The arms of window w are arm indices [first_arm, first_arm + n_internal + n_prefix + n_suffix),
 * stored as internal arms, then prefix arms, then suffix arms, each group in INSERTION order
 * (Window::add_internal/add_prefix/add_suffix, Window.hpp:66-101).  The consumption order
 * (prefix arms reversed, Window.cpp:111) is applied by the callee, as are the dispatch rules of
 * Window::generate_consensus (Window.cpp:44-61).  n_empty = Window::_num_empty (add_empty, :103).
 */
typedef struct HypoWindow {
    uint8_t  type;          /* HYPO_WIN_SHORT / HYPO_WIN_LONG */
    uint8_t  reserved[3];
    uint32_t draft_len;     /* bases */
    uint64_t draft_off;     /* BYTE offset of the 4-bit packed draft in HypoWindowBatch.draft4 */
    uint32_t first_arm;
    uint32_t n_internal;
    uint32_t n_prefix;
    uint32_t n_suffix;
    uint32_t n_empty;
    uint32_t reserved2;
} HypoWindow;               /* 40 bytes */

typedef struct HypoWindowBatch {
    uint32_t          n_windows;
    uint32_t          n_arms;
    const HypoWindow* windows;     /* [n_windows] */
    const uint8_t*    draft4;      /* 4-bit packed drafts (PackedSeq<4>) */
    uint64_t          draft4_bytes;
    const uint64_t*   arm_off;     /* [n_arms] BYTE offset of each 2-bit packed arm in arms2; NULL = the arms lie back to back in
                                      arm order, each on a byte boundary (the offsets are then computed on the device) */
    const uint32_t*   arm_len;     /* [n_arms] bases (0 allowed: skipped like Window.cpp:100,113,124) */
    const uint8_t*    arms2;       /* 2-bit packed arms (PackedSeq<2>) */
    uint64_t          arms2_bytes;
} HypoWindowBatch;

/*
 * Result of Window::get_consensus() (Window.hpp:63) for every window of the batch.
 * The caller owns all buffers.  Slot of window w = bases[off[w] .. off[w+1]); the callee writes
 * len[w] characters (ASCII ACGTN) there, no terminator, and status[w].
 */
typedef struct HypoConsensusBatch {
    char*           bases;
    const uint64_t* off;       /* [n_windows + 1] */
    uint32_t*       len;       /* [n_windows] */
    uint8_t*        status;    /* [n_windows] HYPO_ST_* */
} HypoConsensusBatch;

/* Runtime ------------------------------------------------------------------------------------- */

/* Creates one context (stream, device arenas) per listed HIP device; (NULL, 0) = device 0 only.  The calling thread is left
 * on context 0.  Replaces nothing in the reference (there is no device there); closest analogue Hypo::Hypo,
 * src/Hypo.cpp:34-36.  Calling it again releases the previous contexts first. */
int hypo_gpu_init(const int* device_ids, int n_devices);
int hypo_gpu_shutdown(void);
int hypo_gpu_abi_version(void);
const char* hypo_gpu_last_error(void);
/* Contexts created by hypo_gpu_init (0 before). */
int hypo_gpu_num_devices(void);
/* Makes context `slot` (index into the device list of hypo_gpu_init) the one this THREAD's later calls work on. */
int hypo_gpu_use_device(int slot);
/* Opt-in behaviour switches (all contexts; set before the POA calls they should affect):
 *   "native_klov"  1 = rank the end rows of prefix arms (kLOV) by the maximum over the whole row, as the AVX2 / SSE4.1 alignment
 *                  engine of a -march=native build of the reference does (external/spoa/src/simd_alignment_engine.cpp:803,
 *                  834-840,859-861); 0 (default) = the scalar engine's rule, which the reference's default build uses.
 *   "poa_min_class" 0..3 (default 0): SHORT windows start in at least this size class of the POA kernel.  Results do not depend on it
 *                  (every class computes the reference's consensus); parity sweeps use it to run small windows through the code
 *                  of the larger classes (tests/exhaustive_parity.py).
 *   "giant_arena_mb" megabytes of HBM that size class 6 of the POA kernel gets per POA context created after the call (default 1024): the
 *                  windows beyond the table-driven classes — an arm or draft of more than 1 021 bases, more than 16 382 sequences, more
 *                  than 32 767 nodes — run there with their whole state in a slice of it (two windows at a time), by the reference's own
 *                  procedure with its full score matrix.  A window that needs more than a slice answers HYPO_ST_CAPACITY; 0 = no class 6.
 *   "edit_chunk_mb" 1..4096 (default 256): megabytes of move storage one launch of the long / wide paths of hypo_gpu_edit_scripts may
 *                  use; a list that needs more runs in several launches (a single pair that needs more runs alone).  Results do not
 *                  depend on it; the tests use 1 to run the chunk loop with small inputs. */
int hypo_gpu_set_option(const char* name, int value);
/* First 16 hex digits of the SHA-256 over the library's sources (the .hip and .hpp files of hypo_amd/csrc and this header, in sorted
 * order), embedded at build time: says which sources a prebuilt libhypo_gpu.so came from (tests/test_abi.py checks it). */
const char* hypo_gpu_build_id(void);
/* Number of compute units of the calling thread's device (0 before init). */
int hypo_gpu_num_cus(void);

/* Solid-kmer scan --------------------------------------------------------------------------------
 * Replaces Contig::find_solid_pos (src/Contig.cpp:40-74) + suk::SolidKmers::is_solid
 * (external/suk/include/suk/SolidKmers.hpp:119).
 *   packed4      contig as PackedSeq<4> bytes, n_bases bases
 *   k            2..31 (reference derives 11/13/15/17, src/main.cpp:490-528)
 *   bitset_words 4^k bits as little-endian 64-bit words, bit i at word i>>6, bit i&63
 *                (sdsl::bit_vector payload, external/suk/src/SolidKmers.cpp:47-48,182-186)
 * Outputs:
 *   solid_pos_words  ceil(n_bases/64) words; bit p set <=> Contig::_solid_pos[p] (Contig.cpp:67)
 *   kids             k-mer ids of the marked positions in increasing position order
 *                    (Contig::_kmerinfo[i]->kid, Contig.cpp:68); at most kids_cap are written
 *   word_rank        optional (may be NULL): ceil(n_bases/64)+1 exclusive prefix counts of set bits
 *                    per word = the directory behind sdsl rank_1/select_1 (Contig.cpp:72-73)
 *   n_solid          total number of marked positions (even if > kids_cap)
 * bitset_words == NULL: use the set last uploaded to this context with hypo_gpu_solid_set_upload (same k), so that a run
 * over many contigs sends the 4^k-bit set (2 GiB at k = 17) to the device once, like the reference loads it once
 * (src/Hypo.cpp:70-77).
 */
int hypo_gpu_solid_set_upload(const uint64_t* bitset_words, uint32_t k);
int hypo_gpu_solid_scan(const uint8_t* packed4, uint64_t n_bases, uint32_t k,
                        const uint64_t* bitset_words,
                        uint64_t* solid_pos_words, uint64_t* kids, uint64_t kids_cap,
                        uint64_t* word_rank, uint64_t* n_solid);

/* Same with device pointers; workspace from hypo_gpu_solid_scan_workspace_bytes(n_bases).
 * n_solid is a DEVICE pointer to one uint64. */
size_t hypo_gpu_solid_scan_workspace_bytes(uint64_t n_bases);
int hypo_gpu_solid_scan_device(const uint8_t* packed4, uint64_t n_bases, uint32_t k,
                               const uint64_t* bitset_words,
                               uint64_t* solid_pos_words, uint64_t* kids, uint64_t kids_cap,
                               uint64_t* word_rank, uint64_t* n_solid,
                               void* workspace, size_t workspace_bytes, void* hip_stream);

/* Window POA -------------------------------------------------------------------------------------
 * Replaces Window::prepare_for_poa (src/Window.cpp:31-42) + the per-window loop
 * `generate_consensus(w, omp_get_thread_num())` of src/Hypo.cpp:238-247, i.e.
 * Window::generate_consensus (Window.cpp:44-61), generate_consensus_short (:87-154),
 * generate_consensus_long + curate (:156-254) and the HyPo-adapted spoa underneath
 * (external/spoa/src/sisd_alignment_engine.cpp:246-439, graph.cpp:117-353,467-476,533-568,610-705).
 * Scores must have gap <= 0 (spoa throws otherwise, alignment_engine.cpp:43-50) -> HYPO_E_INVALID.
 * Results are bit-identical to the reference's scalar (SISD) engine.
 */
int hypo_gpu_poa_batch(const HypoScoreParams* scores, const HypoWindowBatch* in,
                       HypoConsensusBatch* out);

/* The same call in two halves, so that two batches can be in flight on one context: _begin queues the upload, the kernels and
 * the download of the results on a stream of its own and returns a ticket without waiting; _end(ticket) waits for that batch
 * (hypo_gpu_poa_last_stats then describes it).  Buffers of `in` and `out` must stay untouched in between; page-locked host
 * buffers (hipHostMalloc / hipHostRegister) make the copies true DMA.  A third _begin before an _end is refused. */
int hypo_gpu_poa_batch_begin(const HypoScoreParams* scores, const HypoWindowBatch* in,
                             HypoConsensusBatch* out, int* ticket);
int hypo_gpu_poa_batch_end(int ticket);

/* The same batch over ALL contexts of hypo_gpu_init (src/Hypo.cpp:238-247 is a parallel loop over independent windows): the
 * window list is cut into one contiguous cost-balanced range per device, every device polishes its range, and the consensus
 * bytes, lengths and status bytes are exchanged with one grouped RCCL all-gatherv (ncclBroadcast per owner) over xGMI, so
 * that device 0 holds the whole result before it returns to the host for contig re-assembly (src/Contig.cpp:345-366).
 * One context: identical to hypo_gpu_poa_batch.  HYPO_MULTI_GATHER=direct skips RCCL (each device copies its range back). */
int hypo_gpu_poa_batch_sharded(const HypoScoreParams* scores, const HypoWindowBatch* in,
                               HypoConsensusBatch* out);

/* Recommended workspace: queues for n_windows plus HBM scratch for as many resident groups of the LONG-window class as the
 * batch could use (up to 2048 x 3.3 MB).  A smaller workspace is accepted down to 16 resident groups (HYPO_E_WORKSPACE
 * below that); it only limits how many LONG / oversized windows are in flight at once. */
size_t hypo_gpu_poa_workspace_bytes(uint32_t n_windows, uint32_t n_arms);
int hypo_gpu_poa_batch_device(const HypoScoreParams* scores, const HypoWindowBatch* in,
                              HypoConsensusBatch* out, void* workspace, size_t workspace_bytes,
                              void* hip_stream);

/* Fills off[0..n_windows] (HOST pointers) with the consensus slot layout the callee recommends:
 * slot(w) = round_up(1.5 * max(draft_len, longest arm) + 24, 8).  Pure host helper.  A consensus that outgrows its slot
 * comes back as HYPO_ST_CONS_OVERFLOW with len = the size it needs (the host mirror then asks again for those windows). */
int hypo_gpu_poa_slot_layout(const HypoWindowBatch* host_in, uint64_t* off);

/* Telemetry of the last POA call on this thread (windows per size class, escalations, DP cells). */
typedef struct HypoPoaStats {
    uint64_t n_windows;
    uint64_t n_trivial;        /* answered by the dispatch rules without POA */
    uint64_t n_class[8];       /* windows finished in size class 0..7 (5 in use) */
    uint64_t n_escalated;      /* windows that overflowed a class and were re-run in the next */
    uint64_t n_failed;         /* status != OK */
    uint64_t dp_cells;         /* sum over alignments of (nodes+1)*(len+1), sisd..cpp:266-267 */
    uint64_t n_alignments;
    uint64_t alg_bytes[8];     /* algorithmic HBM bytes of the windows finished in class 0..7:
                                  ceil(Ld/2) + sum ceil(La/4) + Lcons + 16 + 8*(1+n_arms)   */
    /* How the n_alignments were answered (dp_cells counts every one of them as the reference would compute it): */
    uint64_t n_reused;         /* byte-identical to the alignment just made on an unchanged graph: weights only */
    uint64_t n_threaded;       /* the sequence spells a path of the graph: one-bit recurrence, no scores */
    uint64_t cells_scored;     /* matrix cells that went through the score rows (windows re-run after an overflow included) */
    uint64_t cells_threaded;   /* matrix cells that went through the one-bit rows (failed attempts included) */
    uint64_t n_carried;        /* of n_escalated: re-queued together with the graph of the sequences added so far (ABI 6) */
} HypoPoaStats;
int hypo_gpu_poa_last_stats(HypoPoaStats* out);
/* Same for a _device call: synchronises the stream and copies the counters out of `workspace`. */
int hypo_gpu_poa_read_stats(const void* workspace, void* hip_stream, HypoPoaStats* out);

/* ---- Arm selection on the device ----------------------------------------------------------------------
 * Replaces, for SHORT windows, the host loops that cut every mapped short read at the region borders and hand the pieces
 * to the windows:
 *   Alignment::find_short_arms / find_bp / prepare_short_arm   src/Alignment.cpp:222-259, 321-406, 408-511
 *   Alignment::add_arms + Contig::fill_short_windows (pruning)  src/Alignment.cpp:301-318, src/Contig.cpp:249-289
 * hypo_gpu_arms_build takes the regions of the contigs of one batch and their short-read alignments as flat host arrays,
 * builds the HypoWindowBatch of the surviving windows IN DEVICE MEMORY (arms in alignment order: internal, prefix, suffix)
 * and returns which regions kept a window; hypo_gpu_arms_poa polishes that resident batch (same kernels as
 * hypo_gpu_poa_batch) and returns the consensus sequences; hypo_gpu_arms_download copies the batch to the host (region dump,
 * tests, the rare windows that need the host's retry path).  One resident batch per context; the next build replaces it.
 *
 * Several contigs go over as one coordinate space: the caller concatenates them (each contig starting on an even position,
 * a 1-base filler region of type SR where it pads), shifts rb / re by the contig's offset and the SR ranks in `info` by the
 * number of SRs before the contig.  Alignments must be sorted by rb (a coordinate-sorted BAM; HYPO_E_INVALID otherwise: the
 * arm order inside a window is the alignment order and the kernels rely on the sort to find a window's alignments). */
typedef struct HypoArmsRegions {
    uint32_t        n_regions;
    const uint32_t* start;         /* [n_regions + 1] region starts, then the total length */
    const uint8_t*  type;          /* [n_regions + 1] RegionType (include/globalDefs.hpp:95-108): SWS SW WS MWM MW WM SWM MWS OTHER LONG SR MSR */
    const uint32_t* info;          /* [n_regions + 1] SR: its rank among the SRs; MSR: its minimizer (Contig::_reg_info) */
    uint64_t        n_anchor_kmers;
    const uint64_t* anchor_kmers;  /* [1 + 2 * number of SRs] a dummy, then first and last k-mer of every SR (Contig::_anchor_kmers);
                                      the SR of rank r >= 1 (info) owns entries 2r - 1 and 2r */
    uint32_t        k;
    const uint8_t*  contig4;       /* PackedSeq<4> of the coordinate space */
} HypoArmsRegions;
typedef struct HypoArmsReads {
    uint32_t        n_alignments;
    const uint32_t* rb;            /* reference span [rb, re) (Alignment::_rb, _re) */
    const uint32_t* re;
    const uint32_t* qae;           /* aligned query length, soft clips dropped (Alignment::_qae with _qab = 0) */
    const uint64_t* seq_off;       /* BYTE offset of the aligned query as PackedSeq<2> in reads2 */
    const uint8_t*  reads2;
    uint64_t        reads2_bytes;
    const uint32_t* cigar_off;     /* [n_alignments + 1] */
    const uint32_t* cigar;         /* BAM encoding: len << 4 | op */
    const uint32_t* file_rank;     /* NULL: the alignments are given in file order (a coordinate-sorted file).  Else [n_alignments]:
                                      the position of every alignment in the FILE; the alignments themselves must still come sorted
                                      by rb (the caller sorts an unsorted file's records on ingest), and the arms of a window are
                                      laid out by file_rank — the reference takes them in file order whatever the positions are
                                      (src/Hypo.cpp:314-318, src/Alignment.cpp:301-318), and the POA result depends on that order */
} HypoArmsReads;
typedef struct HypoArmsSummary {
    uint32_t n_windows;            /* windows that survived Contig::fill_short_windows' pruning */
    uint32_t n_arms;
    uint64_t arms2_bytes, draft4_bytes;
    uint64_t out_bytes;            /* consensus slots (hypo_gpu_poa_slot_layout's rule) */
} HypoArmsSummary;
/* region_valid: [n_regions] out, 1 where the region keeps a SHORT window.  HYPO_E_CAPACITY: the batch exceeds the 32-bit
 * counters of the boundary (use the host path or smaller contig batches). */
int hypo_gpu_arms_build(const HypoArmsRegions* regions, const HypoArmsReads* reads /* NULL: the reads of hypo_gpu_reads_upload */, uint8_t* region_valid, HypoArmsSummary* summary);
/* Any pointer may be NULL.  windows [n_windows], win_region [n_windows] (region of every window), arm_len / arm_off [n_arms],
 * arms2 [arms2_bytes], draft4 [draft4_bytes]. */
int hypo_gpu_arms_download(HypoWindow* windows, uint32_t* win_region, uint32_t* arm_len, uint64_t* arm_off, uint8_t* arms2, uint8_t* draft4);
/* bases [out_bytes], off [n_windows + 1] (OUT), len / status [n_windows]; stats through hypo_gpu_poa_last_stats. */
int hypo_gpu_arms_poa(const HypoScoreParams* scores, char* bases, uint64_t* off, uint32_t* len, uint8_t* status);

/* The same for LONG windows (ABI 6): replaces
 *   Alignment::find_long_arms            src/Alignment.cpp:262-299   (the read cut at the borders of the pseudo regions)
 *   Window::add_prefix / add_suffix / add_internal for LONG windows, i.e. Filter::initialise + Filter::is_good
 *                                        include/Window.hpp:66-101, include/Filter.hpp:33-102   (an arm is kept if it shares one
 *                                        canonical (k = 10, w = 10) window minimizer per 50 bases with the window's draft)
 *   Contig::fill_long_windows            include/Contig.hpp:91-113   (prefix / suffix arms dropped above 10 internal arms)
 * `regions` are the PSEUDO regions of Contig::prepare_long_windows (src/Contig.cpp:292-343: start = a set bit of
 * _pseudo_reg_pos, type = SR or LONG, info and the anchor k-mers are not used and may be NULL / 0), `reads` the long-read
 * alignments of the contig batch in file order.  Every LONG pseudo region becomes a window of type HYPO_WIN_LONG
 * (region_valid = 1 there), with or without arms.  The resident LONG batch lives beside the SHORT one of hypo_gpu_arms_build:
 * neither call disturbs the other's batch. */
int hypo_gpu_arms_build_long(const HypoArmsRegions* pseudo_regions, const HypoArmsReads* long_reads, uint8_t* region_valid, HypoArmsSummary* summary);
int hypo_gpu_arms_download_long(HypoWindow* windows, uint32_t* win_region, uint32_t* arm_len, uint64_t* arm_off, uint8_t* arms2, uint8_t* draft4);
int hypo_gpu_arms_poa_long(const HypoScoreParams* scores, char* bases, uint64_t* off, uint32_t* len, uint8_t* status);

/* ---- Support votes on the device (ABI 6) --------------------------------------------------------------------
 * Replaces the two per-alignment loops that count, for every solid k-mer and every mega-window minimizer of the draft, the
 * reads that cover it and the reads that support it:
 *   Alignment::update_solidkmers_support   src/Alignment.cpp:65-132    (mutex per k-mer, include/Contig.hpp:207-214)
 *   Alignment::update_minimisers_support   src/Alignment.cpp:134-220
 * hypo_gpu_reads_upload puts the short-read alignments of a contig batch on the device once (same arrays and coordinate space
 * as hypo_gpu_arms_build; read_contig[a] = index of the read's contig in the batch; total_len = size of the coordinate space);
 * the two support calls vote with that copy, and hypo_gpu_arms_build(regions, NULL, ...) later cuts the same copy into arms.
 * Counters are 32-bit on the device; the reference's are 16-bit and wrap (the host reads them through & 0xffff). */
int hypo_gpu_reads_upload(const HypoArmsReads* reads, const uint32_t* read_contig, uint64_t total_len);
/* spos [n_solid]: positions of the solid k-mers of the coordinate space, ascending (Contig::_solid_pos); kids [n_solid]: their
 * k-mers (KmerInfo::kid).  OUT coverage / support [n_solid] (KmerInfo::coverage / support). */
int hypo_gpu_support_kmers(uint32_t k, uint64_t n_solid, const uint32_t* spos, const uint64_t* kids, uint32_t* coverage, uint32_t* support);
typedef struct HypoMegaWindows {     /* Contig::_reg_pos / _is_win_even / _minimserinfo after prepare_for_division */
    uint32_t        n_contigs;
    const uint32_t* contig_base;     /* [n_contigs] start of the contig in the coordinate space */
    const uint32_t* reg_base;        /* [n_contigs + 1] first entry of the contig in `start` */
    const uint8_t*  win_even;        /* [n_contigs] Contig::_is_win_even */
    const uint32_t* info_base;       /* [n_contigs] index of the contig's first MWMinimiserInfo */
    const uint32_t* start;           /* contig-local region borders (set bits of _reg_pos: 0, SR starts and ends, the length) */
    uint32_t        n_info;
    const uint32_t* mw_off;          /* [n_info + 1] entries of every MWMinimiserInfo */
    const uint32_t* rel_pos;         /* per entry: MWMinimiserInfo::rel_pos */
    const uint32_t* minimisers;      /* per entry: MWMinimiserInfo::minimisers */
} HypoMegaWindows;
/* OUT coverage / support [mw_off[n_info]] (MWMinimiserInfo::coverage / support). */
int hypo_gpu_support_minimizers(const HypoMegaWindows* windows, uint32_t* coverage, uint32_t* support);

/* Round 4 (ABI 7): what only the device reads stays on the device ------------------------------------------------------------------
 * hypo_gpu_solid_scan_keep: hypo_gpu_solid_scan (the 4^k-bit set must have been uploaded with hypo_gpu_solid_set_upload) whose
 * k-mer ids (Contig::_kmerinfo[i]->kid, src/Contig.cpp:68) and marked positions are NOT returned: they stay in device memory under
 * `handle` (the caller's contig number, < 2^24) until hypo_gpu_solid_release(handle) (0xffffffff: every handle of the context) or
 * hypo_gpu_shutdown.  The host gets the mark bits, their rank directory and the count — what Contig::_solid_pos needs; a k-mer id it
 * wants later (the anchors of Contig::prepare_for_division, src/Contig.cpp:117-118,126-127) is the k bases at that position of
 * the contig it already holds.
 * hypo_gpu_support_kmers_kept: hypo_gpu_support_kmers for the kept scans of `n_contigs` contigs laid back to back in the
 * coordinate space of the resident reads at contig_base[c] (ascending): OUT coverage / support, Contig::_kmerinfo counters of
 * contig 0, then contig 1, ... (n_solid_total entries; pass buffers of sum(n_solid) entries).  A handle that holds no scan ON
 * THE CALLING THREAD'S CONTEXT -> HYPO_E_INVALID (the caller then sends positions and k-mers with hypo_gpu_support_kmers). */
int hypo_gpu_solid_scan_keep(uint32_t handle, const uint8_t* packed4, uint64_t n_bases, uint32_t k,
                             uint64_t* solid_pos_words_out, uint64_t* word_rank_out, uint64_t* n_solid_out);
int hypo_gpu_solid_release(uint32_t handle);
int hypo_gpu_support_kmers_kept(uint32_t k, uint32_t n_contigs, const uint32_t* handles, const uint32_t* contig_base,
                                uint32_t* coverage, uint32_t* support, uint64_t* n_solid_total);
/* Page-locked host memory for the caller's staging buffers (reads, result buffers): copies from / into it run at the link's rate
 * and truly asynchronously; pageable memory is staged through the runtime's own bounce buffers.  Any buffer of this header may
 * live in it; none has to. */
int hypo_gpu_host_alloc(size_t bytes, void** out);
int hypo_gpu_host_free(void* p);
/* ABI 8: page-lock memory the caller already has, in place (0.045 s per GB on the MI355X box against 0.18 s per GB + 0.12 s per GB
 * to free for hypo_gpu_host_alloc; copies out of it run at 57 GB/s, out of ordinary memory at 14-25 GB/s through the library's
 * bounce buffers).  Worth it for a staging buffer that is used again: the host pipeline registers one on its second use.  The range
 * must stay allocated until it is unregistered. */
int hypo_gpu_host_register(void* p, size_t bytes);
int hypo_gpu_host_unregister(void* p);

/* ABI 9: the solid k-mer set built from the short reads (replaces KMC -k<k> -ci2 -cs<4c> -cx<4c> and
 * suk::SolidKmers::initialise, external/suk/src/SolidKmers.cpp:68-208; DESIGN.md "Solid k-mers from the reads").
 *  - hypo_gpu_kmer_count_begin(k, c): allocates the context's count table, 4^k counters indexed by the canonical code
 *    min(fwd, rc) (A0 C1 G2 T3, MSB-first), 1 byte each when 4c + 1 <= 255, else 2; k in 5..17, c in 1..HYPO_KMER_MAX_COVERAGE.
 *    A counter stops at 4c + 1, which stands for "above -cx".
 *  - hypo_gpu_kmer_count_add(bytes, n): counts every k-mer of the bytes; any byte other than ACGTacgt ends a run of bases (put
 *    one between two reads).  Calls add up; many small calls count what one large call counts.  Synchronous: `bytes` may be
 *    reused on return (page-locked memory from hypo_gpu_host_alloc is copied at the link's rate).
 *  - hypo_gpu_kmer_histogram(hist, 4c + 1): hist[v] = number of canonical k-mers counted v times, 2 <= v <= 4c (-ci2 -cx<4c>);
 *    hist[0] = hist[1] = 0 (SolidKmers.cpp:129-150).
 *  - hypo_gpu_solid_set_build(lower, upper, exclude_hp, bits, n_bits, n_canonical): for every canonical k-mer with
 *    lower <= count <= upper (and 2 <= count <= 4c), and with exclude_hp no homopolymer at either end (s[0] == s[1] or
 *    s[k-1] == s[k-2]), sets bit fwd and bit rc of the 4^k-bit set (bits: 4^k / 64 host words, all written, sdsl word layout).
 *    n_bits = set bits (SolidKmers.cpp:204), n_canonical = solid canonical k-mers (SolidKmers::get_num_solid_kmers).
 *    The set is left in the context's solid-set buffer as well, but is not "uploaded": call hypo_gpu_solid_set_upload as usual.
 *  - hypo_gpu_kmer_count_end(): frees the table. */
#define HYPO_KMER_MAX_COVERAGE 4095u
int hypo_gpu_kmer_count_begin(uint32_t k, uint32_t coverage);
int hypo_gpu_kmer_count_add(const char* bytes, uint64_t n);
int hypo_gpu_kmer_histogram(uint64_t* hist, uint32_t n_bins);
int hypo_gpu_solid_set_build(uint32_t lower, uint32_t upper, int exclude_hp, uint64_t* bits, uint64_t* n_bits, uint64_t* n_canonical);
int hypo_gpu_kmer_count_end(void);

/* ABI 10: edit scripts of the replacement units (hypo --vcf; DESIGN.md "Edit scripts").  Pair p aligns a[a_off[p], a_off[p+1])
 * (the draft span) against b[b_off[p], b_off[p+1]) (its polished text) with unit costs, bytes compared as bytes; the traceback
 * from (n, m) takes the first move that holds of diagonal, up (a base of `a` deleted), left (a base inserted).
 *  - dist[n_pairs]: the edit distances; run_off[n_pairs + 1]: where each pair's runs start in runs[] (run_off[0] = 0);
 *    runs[] = (len << 2) | op, op 0 '=', 1 'X', 2 'D', 3 'I', in draft order; consecutive runs have different ops.
 *  - runs_cap < run_off[n_pairs]: HYPO_E_WORKSPACE with dist and run_off filled; call again with runs of that size.  The
 *    context keeps the results of that call: the next call on it that names the same batch (the same a, b pointers and the same
 *    offsets; the bytes must not have changed in between) copies them out without computing again.
 *  - every side below 2^30 bytes.  Runs on the calling thread's context; synchronous. */
typedef struct HypoEditBatch {
    uint32_t n_pairs, _pad;
    const char* a; const uint64_t* a_off;
    const char* b; const uint64_t* b_off;
} HypoEditBatch;
int hypo_gpu_edit_scripts(const HypoEditBatch* in, uint32_t* dist, uint64_t* run_off, uint32_t* runs, uint64_t runs_cap);
/* What the last computing hypo_gpu_edit_scripts call on the calling thread's context did (zeros before the first; a call that only
 * copied kept results out after HYPO_E_WORKSPACE leaves it alone).  Additive to ABI 11: bind it by name.
 *   out[0] pairs; out[1] entries of the long list (fast band, move codes in device memory); out[2] entries of the wide list (pairs the
 *   fast band could not decide, and probes of pairs with |m - n| > 127); out[3] entries of the second wide list (probes that were not
 *   exact); out[4] runs written; out[5] passes over the run pool (2: the pool was too small and the call ran again with the size it
 *   had counted); out[6], out[7]: launches of the long and of the wide kernel in the last pass (one per chunk of "edit_chunk_mb").
 * All of them are numbers the host loop holds; the routing itself is in DESIGN.md "Edit scripts". */
int hypo_gpu_edit_last_counts(uint64_t out[8]);

/* ABI 11: an exact set of the canonical k-mers of the reads, and how many k-mers of a sequence it lacks (hypo --qv; DESIGN.md
 * "k-mer QV").  A hash table in device memory on the calling thread's context: presence only, no false positives.
 *  - hypo_gpu_kset_begin(k, expected_distinct, max_bytes): k in 12..31.  The table is sized for expected_distinct keys at a load
 *    of one half (at least 1024 slots of 8 bytes) and never grows beyond max_bytes (0: half of the memory the device had free at
 *    hypo_gpu_init).
 *  - hypo_gpu_kset_add(bytes, n): inserts min(fwd, rc) (A0 C1 G2 T3, MSB-first) of every k-mer of the bytes; the byte rules and the
 *    guarantee about splitting the input into calls are those of hypo_gpu_kmer_count_add (overlap the calls by k - 1 bytes; a
 *    larger overlap changes nothing here).  Synchronous.  Before it touches the table the call makes room for its worst case,
 *    n - k + 1 new keys, by moving the keys into a larger table; when max_bytes does not allow that it returns HYPO_E_CAPACITY
 *    (hypo_gpu_last_error names the size reached) and the set is what it was before the call.
 *  - hypo_gpu_kset_size(n_distinct, table_bytes): keys in the set, bytes of the table (either pointer may be NULL).
 *  - hypo_gpu_kset_query(bytes, off, n_seqs, total, missing): sequence s is bytes[off[s], off[s + 1]); total[s] = its length-k
 *    windows made of ACGTacgt only, missing[s] = those, with multiplicity, whose canonical k-mer is not in the set.
 *  - hypo_gpu_kset_end(): frees the table and the buffers.
 * add / size / query without begin: HYPO_E_INVALID. */
int hypo_gpu_kset_begin(uint32_t k, uint64_t expected_distinct, uint64_t max_bytes);
int hypo_gpu_kset_add(const char* bytes, uint64_t n);
int hypo_gpu_kset_size(uint64_t* n_distinct, uint64_t* table_bytes);
int hypo_gpu_kset_query(const char* bytes, const uint64_t* off, uint32_t n_seqs, uint64_t* total, uint64_t* missing);
int hypo_gpu_kset_end(void);
/* Many short spans of one text against the set (hypo --kmer-guard; DESIGN.md "k-mer guard").  Additive to ABI 11: callers bind it
 * by name.  Span s is bytes[lo[s], hi[s]); total[s] = its length-k windows made of ACGTacgt only, missing[s] = those, with
 * multiplicity, whose canonical k-mer is not in the set (the byte rules of hypo_gpu_kset_query).  No window crosses a span's ends.
 * Spans may overlap, repeat, be empty or shorter than k, and come in any order; the answers depend on the input alone.  All
 * n_bytes are sent to the device once, whatever the spans cover.  lo[s] > hi[s] or hi[s] > n_bytes: HYPO_E_INVALID.  Without a
 * set: HYPO_E_INVALID, as hypo_gpu_kset_query.  Synchronous, on the calling thread's context. */
int hypo_gpu_kset_query_spans(const char* bytes, uint64_t n_bytes, const uint64_t* lo, const uint64_t* hi, uint32_t n_spans, uint64_t* total, uint64_t* missing);
/* Every subset of a few edits of many short sites against the set (hypo --guard-records; DESIGN.md "k-mer guard by record").
 * Additive to ABI 11: callers bind it by name.  Site s is bytes[lo[s], hi[s]); its edits are e in [edit_off[s], edit_off[s + 1]),
 * at most HYPO_KSET_MAX_EDITS of them (none is allowed); edit e replaces bytes[eb[e], ee[e]) by alts[ao[e], ao[e] + al[e]).  Inside
 * a site the edits ascend and do not overlap: lo <= eb_0 <= ee_0 <= eb_1 <= ... <= ee_{n-1} <= hi; abutting edits, empty REF
 * spans and empty ALTs are allowed.  Variant m of a site (m < 2^n) is its text with the ALT of edit j where bit j of m is set and
 * the REF bytes elsewhere; total / missing of a variant are those of hypo_gpu_kset_query for that text (no window crosses the
 * site's ends).  The variants' texts are never built.  best_mask[s] is the variant with the fewest missing windows, among those
 * the one with the most bits set, among those the greatest m; best_total[s] / best_missing[s] are its pair.  var_total /
 * var_missing (each may be NULL) receive every variant's pair: in site order, within a site in mask order, sum of 2^n entries.
 * Sites may overlap, repeat and come in any order; the answers depend on the input alone.  HYPO_E_INVALID: edits out of order or
 * out of range, more than HYPO_KSET_MAX_EDITS of them in a site, a variant of 2^31 bytes or more, more than 2^32 - 1 variants in
 * the call, a NULL required pointer with n_sites > 0, no set (as hypo_gpu_kset_query); a refused call changes nothing.
 * Synchronous, on the calling thread's context. */
#define HYPO_KSET_MAX_EDITS 12
int hypo_gpu_kset_query_variants(const char* bytes, uint64_t n_bytes, const char* alts, uint64_t n_alt_bytes,
    const uint64_t* lo, const uint64_t* hi, const uint32_t* edit_off /* n_sites + 1 */, uint32_t n_sites,
    const uint64_t* eb, const uint64_t* ee, const uint64_t* ao, const uint32_t* al,
    uint32_t* best_mask, uint64_t* best_total, uint64_t* best_missing,
    uint64_t* var_total /* may be NULL */, uint64_t* var_missing /* may be NULL */);
/* hypo_gpu_kset_query, and WHERE the missing windows are (hypo --qv-bed; DESIGN.md "k-mer QV track").  Additive to ABI 11: callers
 * bind it by name.  bytes, off, n_seqs, total and missing are those of hypo_gpu_kset_query and receive the same values.  A base of
 * a sequence is covered when a missing window contains it; the intervals of a sequence are its maximal runs of covered bases
 * [start, end), relative to off[s], so missing windows that overlap or abut share one, end - start >= k, and start[j + 1] > end[j].
 * An interval never joins two sequences.  iv_missing = the missing windows that start in [start, end - k]; over a sequence they add
 * up to missing[s].  want (NULL: every sequence): want[s] == 0 gives sequence s no intervals; total and missing do not depend on
 * it.  iv_off[n_seqs + 1] (iv_off[0] = 0): the intervals of s are [iv_off[s], iv_off[s + 1]) of iv_start / iv_end / iv_missing, in
 * ascending order.  iv_off[n_seqs] > iv_cap: HYPO_E_WORKSPACE with total, missing and iv_off filled and the three arrays untouched;
 * call again with room.  iv_cap == 0 (the three pointers may then be NULL) is the counting call; it returns 0 when there is no
 * interval.  HYPO_E_INVALID: off[] decreasing, a NULL required pointer with n_seqs > 0, no set (as hypo_gpu_kset_query); a refused
 * call changes nothing.  The answer is a function of the input alone.  Synchronous, on the calling thread's context. */
int hypo_gpu_kset_query_track(const char* bytes, const uint64_t* off, uint32_t n_seqs, const uint8_t* want /* may be NULL */,
    uint64_t* total, uint64_t* missing, uint64_t* iv_off /* n_seqs + 1 */,
    uint64_t* iv_start, uint64_t* iv_end, uint64_t* iv_missing, uint64_t iv_cap);
/* Every one-base edit of many short regions against the set (hypo --kmer-fix; DESIGN.md "k-mer fix").  Additive to ABI 11: callers
 * bind it by name.  Site s is the span bytes[lo[s], hi[s]) with the region [c0[s], c1[s]) inside it, w = c1 - c0 bytes wide.  It has
 * 9 w - 3 candidates, in this order: index 0 the span as it is; then sub(p, b), p ascending over the region, b in ACGT order (4 w);
 * then del(p), p ascending over the region (w); then ins(p, b), b put in front of p, p ascending over (c0, c1), b in ACGT order
 * (4 (w - 1)).  Substituted and inserted bytes are upper case.  A candidate's total / missing are those of hypo_gpu_kset_query for
 * the span with that one edit (no window crosses the span's ends; a window holding a non-base byte is no window); the texts are
 * never built.  Different candidates can spell one text; with bases compared case-blind a candidate is CANONICAL when it is
 * sub(p, b) and upper(bytes[p]) != b, or del(p) and p == c0 or upper(bytes[p - 1]) != upper(bytes[p]), or ins(p, b) and p == c0 + 1
 * or upper(bytes[p - 1]) != b; index 0 is not.  Distinct canonical candidates have distinct texts, and every other candidate's text
 * is that of index 0 or of a canonical one.  none_total[s] / none_missing[s]: the pair of index 0.  best_cand[s]: the index of the
 * canonical candidate with the fewest missing windows, the first in order among equals; best_total[s] / best_missing[s]: its pair.
 * zeros[s]: the canonical candidates with no missing window.  cand_total / cand_missing (both given or both NULL) receive every
 * candidate's pair, site s at the sum of 9 w - 3 over the sites before it.  Sites may overlap, repeat and come in any order; the
 * answers depend on the input and the set alone.  HYPO_E_INVALID: lo <= c0 < c1 <= hi <= n_bytes violated, c1 - c0 above
 * HYPO_KSET_MAX_FIX_REGION, hi - lo above HYPO_KSET_MAX_FIX_SPAN, a NULL required pointer with n_sites > 0, one of cand_* without
 * the other, no set (as hypo_gpu_kset_query); a refused call changes nothing.  n_sites == 0 touches nothing.  Synchronous, on the
 * calling thread's context. */
#define HYPO_KSET_MAX_FIX_REGION 31
#define HYPO_KSET_MAX_FIX_SPAN 2048
int hypo_gpu_kset_query_fixes(const char* bytes, uint64_t n_bytes, const uint64_t* lo, const uint64_t* hi,
                              const uint64_t* c0, const uint64_t* c1, uint32_t n_sites,
                              uint64_t* none_total, uint64_t* none_missing, uint32_t* best_cand, uint64_t* best_total,
                              uint64_t* best_missing, uint32_t* zeros,
                              uint64_t* cand_total /* may be NULL */, uint64_t* cand_missing /* may be NULL */);
/* Walks through the set as a de Bruijn graph (hypo --kmer-bridge; DESIGN.md "k-mer bridge").  Additive to ABI 11: callers bind it by
 * name.  A general primitive: it knows nothing of intervals.  Site s has the left anchor L = bytes[from[s], from[s] + k) and the
 * right anchor R = bytes[to[s], to[s] + k), k the set's; case is ignored.  A k-mer x has up to four children y = x[1:] + b, b in
 * ACGT order, those whose canonical k-mer is in the set (under hypo_gpu_kset_min_count: in R_t, as for the other queries).  The
 * answer is the result of this search and nothing else:
 *     steps = found = 0
 *     visit(x, depth, path):
 *         steps += 1;  if steps > budget: stop with BUDGET
 *         if depth >= dlo and x == R:                 (forward strings compared)
 *             found += 1;  if found == 2: stop with AMBIGUOUS
 *             first = path;  return                   (a walk ends at its first allowed arrival)
 *         if depth == dhi: return
 *         for b in A, C, G, T:  y = x[1:] + b;  if canonical(y) in the set: visit(y, depth + 1, path + b)
 *     visit(L, 0, "");  status = UNIQUE if found == 1 else NONE
 * L itself need not be in the set; R must be, or no walk arrives.  A k-mer may be visited more than once: cycles are bounded by dhi.
 * status[s]: one of HYPO_WALK_*; NOANCHOR: an anchor holds a byte outside ACGTacgt.  steps[s]: the counter when the search ended,
 * budget + 1 for BUDGET, 0 for NOANCHOR.  len[s]: for UNIQUE and AMBIGUOUS the first walk's number of steps, its bases written as
 * ACGT bytes at walk[s * HYPO_KSET_MAX_WALK, + len[s]); 0 for NONE, BUDGET and NOANCHOR.  Bytes of walk beyond len are unspecified.
 * Sites may repeat, overlap and come in any order; the answers depend on the input and the set alone.  HYPO_E_INVALID: from + k or
 * to + k beyond n_bytes, dlo < 1, dlo > dhi, dhi > HYPO_KSET_MAX_WALK, budget == 0 or above HYPO_KSET_MAX_WALK_BUDGET, a NULL
 * pointer with n_sites > 0, no set (as hypo_gpu_kset_query); a refused call changes nothing.  n_sites == 0 touches nothing.
 * Synchronous, on the calling thread's context. */
#define HYPO_KSET_MAX_WALK        256     /* largest dhi */
#define HYPO_KSET_MAX_WALK_BUDGET 65536
#define HYPO_WALK_NONE 0
#define HYPO_WALK_UNIQUE 1
#define HYPO_WALK_AMBIGUOUS 2
#define HYPO_WALK_BUDGET 3
#define HYPO_WALK_NOANCHOR 4
int hypo_gpu_kset_query_walks(const char* bytes, uint64_t n_bytes, const uint64_t* from, const uint64_t* to,
                              const uint32_t* dlo, const uint32_t* dhi, uint32_t n_sites, uint32_t budget,
                              uint32_t* status, uint32_t* steps, uint32_t* len, uint8_t* walk);
/* Up to W = HYPO_KSET_MAX_WALKS walks between two anchors, each with its support (hypo --kmer-bridge-vote; DESIGN.md "k-mer bridge
 * vote").  Additive to ABI 11: callers bind it by name.  The set must count (hypo_gpu_kset_counts_enable).  The anchors, the byte
 * rules, the children in ACGT order and the limits on dlo, dhi and budget are those of hypo_gpu_kset_query_walks.  count(y) is the
 * count byte of y's canonical k-mer, 0 when the set does not hold it; t is the least count in force (hypo_gpu_kset_min_count), 1
 * otherwise.  The answer is the result of this search and nothing else:
 *     steps = 0; walks = []
 *     visit(x, depth, path, lo):
 *         steps += 1;  if steps > budget: stop with BUDGET
 *         if depth >= dlo and x == R:                 (forward strings compared)
 *             if len(walks) == W: stop with MANY
 *             walks.append((path, lo));  return       (a walk ends at its first allowed arrival)
 *         if depth == dhi: return
 *         for b in A, C, G, T:  y = x[1:] + b;  c = count(y);  if c >= t: visit(y, depth + 1, path + b, min(lo, c))
 *     visit(L, 0, "", 255)
 *     status = NONE / UNIQUE / AMBIGUOUS for 0 / 1 / 2..W walks
 * The low of a walk is thus the smallest count among the k-mers at its depths 1 .. len: R is included, L is not, and counts stop at
 * 255.  n_walks[s]: the walks reported, in the order of arrival; walk w of site s has len[s * W + w], low[s * W + w] and its bases as
 * ACGT bytes at walk[(s * W + w) * HYPO_KSET_MAX_WALK, + len).  MANY (a walk beyond the Wth arrived) reports the first W; BUDGET and
 * NOANCHOR report n_walks = 0.  status[s] and steps[s] are as for hypo_gpu_kset_query_walks: budget + 1 steps for BUDGET, 0 for
 * NOANCHOR.  Bytes beyond a walk's len and the slots beyond n_walks are left as the caller had them.  Where neither search ends on
 * BUDGET, the first walk here is hypo_gpu_kset_query_walks' and NONE / UNIQUE agree.  HYPO_E_INVALID: everything
 * hypo_gpu_kset_query_walks refuses, and a set that keeps no counts; a refused call changes nothing.  n_sites == 0 touches nothing.
 * Synchronous, on the calling thread's context. */
#define HYPO_KSET_MAX_WALKS 4
#define HYPO_WALK_MANY 5
int hypo_gpu_kset_query_walk_sets(const char* bytes, uint64_t n_bytes, const uint64_t* from, const uint64_t* to,
                                  const uint32_t* dlo, const uint32_t* dhi, uint32_t n_sites, uint32_t budget,
                                  uint32_t* status, uint32_t* steps, uint32_t* n_walks,
                                  uint32_t* len  /* [n_sites * 4] */, uint32_t* low /* [n_sites * 4] */,
                                  uint8_t* walk  /* [n_sites * 4 * HYPO_KSET_MAX_WALK] */);

/* Read k-mer counts and copy numbers on the set (hypo --qv-spectra; DESIGN.md "k-mer spectra").  Additive to ABI 11: callers bind
 * the three by name.  Presence, and with it every answer of the query entry points above, is what it is without them.
 *  - hypo_gpu_kset_counts_enable(n_texts), n_texts in 1..HYPO_KSET_MAX_TEXTS: after hypo_gpu_kset_begin, while the set is empty.
 *    Every slot gets one count byte and n_texts copy bytes; max_bytes of _begin now caps 9 + n_texts bytes a slot (the empty table
 *    is replaced, by a smaller one when the cap asks for it), and hypo_gpu_kset_size reports all resident bytes.  From here on
 *    hypo_gpu_kset_add also counts: every length-k window of the bytes adds 1 to the count of its canonical k-mer, which stops at
 *    255.  A window handed in by two calls is counted twice, so consecutive chunks of one stream of reads must overlap by EXACTLY
 *    k - 1 bytes.  Growth keeps the counts; a call refused with HYPO_E_CAPACITY leaves keys and counts as they were.
 *  - hypo_gpu_kset_mark(text, bytes, off, n_seqs, n_windows, n_unmarked), text < n_texts: the sequences and the byte rules of
 *    hypo_gpu_kset_query.  Every window whose k-mer is in the set adds 1 to that k-mer's copy byte of `text`, which stops at 255;
 *    the other windows are counted in *n_unmarked (it equals the sum of hypo_gpu_kset_query's missing[]), all windows in
 *    *n_windows (either pointer may be NULL).  Calls add up.  An accepted call closes the set: hypo_gpu_kset_add answers
 *    HYPO_E_INVALID from then on.
 *  - hypo_gpu_kset_spectrum(text, hist): hist[c * 5 + j], c = 0..255, j = 0..4, = the k-mers of the set with count c and
 *    min(copy byte of `text`, 4) == j; HYPO_KSET_SPECTRUM_BINS values.  Row 0 is all zero, row 255 means 255 or more, column 4
 *    means 4 or more.
 * HYPO_E_INVALID: no set, _enable on a set that holds k-mers or counts already, n_texts out of range, _mark / _spectrum without
 * _enable or with text >= n_texts, off[] decreasing, a NULL required pointer; a refused call changes nothing.  Synchronous, on the
 * calling thread's context. */
#define HYPO_KSET_MAX_TEXTS 4
#define HYPO_KSET_SPECTRUM_BINS 1280
int hypo_gpu_kset_counts_enable(uint32_t n_texts);
int hypo_gpu_kset_mark(uint32_t text, const char* bytes, const uint64_t* off, uint32_t n_seqs, uint64_t* n_windows, uint64_t* n_unmarked);
int hypo_gpu_kset_spectrum(uint32_t text, uint64_t* hist);
/* A least count for the queries (hypo --qv-min-count; DESIGN.md "k-mer min count").  Additive to ABI 11: callers bind it by name.
 * R_t = the k-mers of the set whose count (hypo_gpu_kset_counts_enable) is at least t; R_1 is the set.  From the next call on
 * hypo_gpu_kset_query, _query_spans, _query_variants, _query_track, _query_fixes and _query_walks answer against R_t: a window whose k-mer the reads contain
 * fewer than t times is missing, and everything those entry points derive from "missing" (intervals, best masks) follows.  The
 * threshold is applied when a query runs, to the counts of that moment: it may be set any number of times, before or after adds
 * and marks, it does not close the set, and hypo_gpu_kset_add, _size, _mark and _spectrum do not know of it.  hypo_gpu_kset_begin
 * starts at t = 1, and with t = 1 the queries run the kernels they run on a set that does not count.  A count stops at 255, so
 * R_255 holds the k-mers seen 255 times or more.  HYPO_E_INVALID: no set, a set without counts, t outside 1..255; a refused call
 * changes nothing.  On the calling thread's context. */
int hypo_gpu_kset_min_count(uint32_t t);
/* Read count against copy number along a text, bin by bin (hypo --qv-cn; DESIGN.md "k-mer copy number").  Additive to ABI 11:
 * callers bind it by name.  The set must count (hypo_gpu_kset_counts_enable) and plane `text` should hold the marks of the whole
 * text the caller compares against (hypo_gpu_kset_mark).  bytes, off, n_seqs and the byte rules are those of hypo_gpu_kset_query.
 * Sequence s, of length L_s = off[s + 1] - off[s], has ceil(L_s / bin) bins; bin j of s owns the length-k windows that START in
 * [j bin, (j + 1) bin) relative to off[s].  Bins are numbered sequence by sequence, and each of the six arrays has n_bins = the sum
 * of ceil(L_s / bin) entries: the caller computes n_bins, and a value that disagrees is refused.  For a window, c is the count byte
 * of its k-mer, m its copy byte of plane `text`, t the least count in force (hypo_gpu_kset_min_count, 1 otherwise).  Per bin:
 *  - windows:   its windows made of ACGTacgt only;
 *  - missing:   those whose k-mer is not in the set or has c < t (over a sequence they add up to hypo_gpu_kset_query's missing[s]);
 *               the present windows are the others;
 *  - rated:     the present windows with 1 <= m <= 254 and c <= 254 (a byte at 255 says "at least"; m = 0: the text was not marked);
 *  - over:      the rated windows with 2 c >= 3 unit m  (the reads hold the k-mer 1.5 times as often as m copies at `unit` each ask);
 *  - under:     the rated windows with 4 c <= 3 unit m  (0.75 times); over and under are disjoint, and every product fits 32 bits;
 *  - med_count: the lower median of c over the present windows, the least v with #{c <= v} >= ceil(present / 2); 0 without one.
 * A bin without a window gets zeros in all six, and every entry is written.  The call does not close the set and changes no byte of
 * it; the answer is a function of the input, the planes and t alone.  HYPO_E_INVALID: no set, a set without counts, text not below
 * the n_texts of _counts_enable, bin outside HYPO_KSET_DEPTH_MIN_BIN .. HYPO_KSET_DEPTH_MAX_BIN, unit outside 1..255, off[]
 * decreasing, n_bins other than the sum above (or 2^32 and more), a NULL required pointer with n_bins > 0; a refused call changes
 * nothing.  n_seqs == 0 touches nothing.  Synchronous, on the calling thread's context. */
#define HYPO_KSET_DEPTH_MIN_BIN 32
#define HYPO_KSET_DEPTH_MAX_BIN 65536
int hypo_gpu_kset_query_depth(const char* bytes, const uint64_t* off, uint32_t n_seqs,
    uint32_t bin, uint32_t text, uint32_t unit, uint64_t n_bins,
    uint32_t* windows, uint32_t* missing, uint32_t* rated, uint32_t* over, uint32_t* under, uint8_t* med_count);
/* The set's records out of the table and back in (hypo --qv-save / --qv-load; DESIGN.md "k-mer set file").  Additive to ABI 11:
 * callers bind them by name.  A record is a canonical code as the table stores it (min(fwd, rc), A0 C1 G2 T3, MSB-first, below
 * 4^k) and a count byte: 1..255 on a set that counts (hypo_gpu_kset_counts_enable), 1 on a set that does not.  The digest of a
 * record is mix64(key) + count * 0x9e3779b97f4a7c15 (mod 2^64), where mix64 is the finaliser of MurmurHash3,
 *     x ^= x >> 33; x *= 0xff51afd7ed558ccd; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53; x ^= x >> 33;
 * and the digest of a list is the sum of its records' digests (mod 2^64): it does not depend on their order.
 *  - hypo_gpu_kset_export(cursor, keys, counts, cap, n_out, digest): a sequence of calls starts with *cursor == 0 and ends when a
 *    call leaves HYPO_KSET_EXPORT_END in it (a call that finds it there writes *n_out = 0).  A call writes *n_out <= cap records
 *    into keys[] and, unless it is NULL, counts[], and moves the cursor on; it may return fewer than cap, even none, before the
 *    end.  Entries at and beyond *n_out are not written.  Over an unchanged set every record comes from exactly one call of the
 *    sequence and the *n_out add up to hypo_gpu_kset_size's n_distinct; the answer is a function of the table, so two sequences
 *    with the same caps return identical arrays.  With digest != NULL the digest of the call's records, summed on the device, is
 *    added to *digest.  The copy bytes of hypo_gpu_kset_mark are not exported; a closed set exports as an open one.  Changing the
 *    set between two calls of a sequence leaves open which records come, and nothing else.  HYPO_E_INVALID: a NULL cursor, keys or
 *    n_out; cap == 0 or cap >= 2^32; a cursor that is neither 0, nor below the table's end, nor what a call handed back; no set.
 *  - hypo_gpu_kset_import(keys, counts, n, digest): for each i < n, keys[i] enters the set if it is absent, and on a set that
 *    counts its count becomes min(255, count + counts[i]) (counts == NULL: 1 each).  The same key several times, in one call or in
 *    several, adds up: the exports of two halves of a read stream, imported one after the other, give the set and the counts of
 *    the whole stream.  A set that does not count checks the counts and otherwise ignores them.  Before the table is touched
 *    every record is checked on the device: keys[i] < 4^k, keys[i] <= its reverse complement, counts[i] >= 1; a violation is
 *    HYPO_E_INVALID, hypo_gpu_last_error names the least offending index, and the set stays as it was.  Room for n new keys is
 *    made as hypo_gpu_kset_add makes it, the counts move with a growth, and HYPO_E_CAPACITY leaves the set as it was.  With digest
 *    != NULL the digest of the n records as given (not as merged) is added to *digest.  HYPO_E_INVALID also: a closed set (as
 *    hypo_gpu_kset_add), n >= 2^32, NULL keys with n > 0, no set.  n == 0 touches nothing.
 * A refused call changes nothing.  Both are synchronous and run on the calling thread's context. */
#define HYPO_KSET_EXPORT_END 0xffffffffffffffffull
int hypo_gpu_kset_export(uint64_t* cursor, uint64_t* keys, uint8_t* counts /* may be NULL */,
                         uint64_t cap, uint64_t* n_out, uint64_t* digest /* may be NULL */);
int hypo_gpu_kset_import(const uint64_t* keys, const uint8_t* counts /* NULL: 1 each */,
                         uint64_t n, uint64_t* digest /* may be NULL */);

/* Kernel timing: each kernel's own start and end time --------------------------------------------
 * hypo_gpu_profile_begin(max_calls) arms the next max_calls (<= 256) *_device calls: each binds HIP
 * events to the dispatches of its kernels (no marker packet on any stream: what a profiled call puts
 * between its kernels is what an unprofiled one does).  hypo_gpu_profile_read(call, ms, n) waits for
 * that call's last kernel and returns up to n elapsed times in milliseconds:
 *   POA call : ms[0] = plan kernels (start of the first to end of the last), ms[1 + c] = the timed launch of size
 *              class c, start to end (6 classes; the LDS classes overlap in time; 0.0 when the call had no such launch),
 *              ms[7] = start of the plan to the end of the call's last kernel (HYPO_PROFILE_POA_SLOTS values)
 *   scan call: ms[0] = the scan kernel, start to end, ms[1] = ms[2] = 0.0 (HYPO_PROFILE_SCAN_SLOTS values)
 * Returns the number of values written, or <0. */
#define HYPO_PROFILE_POA_SLOTS 8
#define HYPO_PROFILE_SCAN_SLOTS 3
int hypo_gpu_profile_begin(int max_calls);
int hypo_gpu_profile_calls(void);
int hypo_gpu_profile_read(int call, float* ms, int n);

#ifdef __cplusplus
}
#endif
#endif /* HYPO_GPU_H */
