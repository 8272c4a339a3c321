// CtxPlan.hpp — which device context works on which contigs of a batch (Hypo::plan_batch): arithmetic on read counts and contig
// lengths only, so that it can be checked without a device (hypo_host_plan_contexts, tests/test_ctx_plan_cpu.py).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace hypo {

// contigs [c0, c1) of the draft; piece: the context owns [own0, own1) of the ONE contig c0 (DeviceArms::set_piece)
struct CtxWork { uint32_t c0 = 0, c1 = 0; bool piece = false; uint32_t own0 = 0, own1 = 0; };

// With several devices the contigs of the batch are dealt out to the contexts in contiguous ranges of about equal
// numbers of alignments: every context keeps the reads of its contigs, counts their support votes, cuts their arms and
// polishes its own resident windows; no window travels.  A batch with FEWER contigs than contexts (BASELINE config C4 is one
// 250 Mbp contig) shares its contigs out instead (round 4): a contig's contexts each own a coordinate range of it and work
// on the reads around that range (DeviceArms::set_piece) — the reference's loop is over the windows of ONE contig too
// (src/Hypo.cpp:236-248).
// n_reads, contig_len: per contig of the batch [initial_cid, final_cid).  split_batch: several contexts and no --host-arms;
// allow_pieces: the device library keeps reads resident and HYPO_NO_PIECES is not set (asked only when pieces are the case).
// Neither: context 0 takes the whole batch.
inline std::vector<CtxWork> plan_contexts(uint32_t initial_cid, uint32_t final_cid, int n_ctx, const uint64_t* n_reads, const uint32_t* contig_len,
                                          bool split_batch, bool allow_pieces) {
    std::vector<CtxWork> work((size_t)n_ctx);
    const uint32_t n_batch_contigs = final_cid - initial_cid;
    work[0].c0 = initial_cid; work[0].c1 = final_cid;
    if (split_batch && n_batch_contigs >= (uint32_t)n_ctx) {
        std::vector<uint32_t> ctx_cut((size_t)n_ctx + 1, final_cid);
        ctx_cut[0] = initial_cid;
        uint64_t total = 0, acc = 0;
        for (uint32_t c = initial_cid; c < final_cid; ++c) total += n_reads[c - initial_cid] + 1;
        int d = 1;
        for (uint32_t c = initial_cid; c < final_cid && d < n_ctx; ++c) {
            acc += n_reads[c - initial_cid] + 1;
            // the cut behind contig c belongs to context d when the first d shares are full (every context gets >= 1 contig)
            while (d < n_ctx && acc * (uint64_t)n_ctx >= total * (uint64_t)d && final_cid - (c + 1) >= (uint32_t)(n_ctx - d)) ctx_cut[(size_t)d++] = c + 1;
        }
        for (; d < n_ctx; ++d) ctx_cut[(size_t)d] = std::max(ctx_cut[(size_t)d - 1] + 1, final_cid - (uint32_t)(n_ctx - d));
        for (int x = 0; x < n_ctx; ++x) { work[(size_t)x].c0 = ctx_cut[(size_t)x]; work[(size_t)x].c1 = ctx_cut[(size_t)x + 1]; }
    } else if (split_batch && allow_pieces) {
        // contexts per contig: one each, the rest one at a time to the contig with most alignments per context it has
        std::vector<uint32_t> share(n_batch_contigs, 1);
        for (uint32_t extra = (uint32_t)n_ctx - n_batch_contigs; extra > 0; --extra) {
            uint32_t best = 0; double best_load = -1;
            for (uint32_t i = 0; i < n_batch_contigs; ++i) {
                const double load = (double)(n_reads[i] + 1) / share[i];
                if (load > best_load) { best_load = load; best = i; }
            }
            ++share[best];
        }
        int d = 0;
        for (uint32_t i = 0; i < n_batch_contigs; ++i) {
            const uint32_t c = initial_cid + i, len = contig_len[i];
            for (uint32_t j = 0; j < share[i]; ++j, ++d) {
                CtxWork& w = work[(size_t)d];
                w.c0 = c; w.c1 = c + 1; w.piece = share[i] > 1;
                w.own0 = (uint32_t)((uint64_t)len * j / share[i]); w.own1 = j + 1 == share[i] ? len : (uint32_t)((uint64_t)len * (j + 1) / share[i]);
            }
        }
    }
    return work;
}

}  // namespace hypo
