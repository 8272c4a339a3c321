// EditVcf.hpp — hypo --vcf: the edits a run made, as VCF records beside the polished FASTA (DESIGN.md "Edit scripts").  The units
// of a contig batch (Contig::collect_units) are aligned on the device in one hypo_gpu_edit_scripts call (edit_kernel.hip); the
// writer thread turns each contig's scripts into records.
#pragma once
#include <cstdint>
#include <memory>
#include <ostream>
#include <string>
#include <vector>
#include "Contig.hpp"

namespace hypo {

using EditScriptsFn = int (*)(const HypoEditBatch*, uint32_t*, uint64_t*, uint32_t*, uint64_t);
// hypo_gpu_edit_scripts, bound by name: only runs with --vcf need it (nullptr: the device library does not provide it)
EditScriptsFn bind_edit_scripts();

struct EditBatchResult {
    std::vector<std::vector<EditUnit>> units;       // per contig of the batch
    std::vector<uint64_t> first;                    // per contig: index of its first unit in the call
    std::vector<uint64_t> run_off;                  // per unit of the call (+ 1)
    std::vector<uint32_t> runs;                     // (len << 2) | op, op 0 '=', 1 'X', 2 'D', 3 'I'
};
// the units of contigs [c0, c1) and their edit scripts (one call on the calling thread's context); HYPO_OK or the C-ABI's error
int edit_scripts_for(EditScriptsFn fn, const std::vector<std::unique_ptr<Contig>>& contigs, uint32_t c0, uint32_t c1, EditBatchResult& out);

struct VcfStats { uint64_t records = 0, sub = 0, ins = 0, del = 0; };
// kmer_filter: the header also declares FILTER kmer (hypo --kmer-guard)
void vcf_header(std::ostream& os, const std::string& reference, const std::vector<std::unique_ptr<Contig>>& contigs, bool kmer_filter = false);
// One record: REF = draft [rb, re), ALT = alt.  whole_del: the contig is written as nothing, its only record is the <DEL> one.
struct VcfRec { uint64_t rb = 0, re = 0; std::string alt; };
struct VcfContigRecords { std::vector<VcfRec> recs; bool whole_del = false; };
// the records of one contig (before Contig::release_after_output); ci = the contig's index in the batch
void vcf_make_records(const Contig& ctg, const EditBatchResult& eb, size_t ci, VcfStats& st, VcfContigRecords& out);
// their lines; rejected (per record, may be NULL): FILTER kmer instead of PASS
void vcf_write_records(std::ostream& os, const Contig& ctg, const VcfContigRecords& rs, const std::vector<uint8_t>* rejected);
// both steps
void vcf_records(std::ostream& os, const Contig& ctg, const EditBatchResult& eb, size_t ci, VcfStats& st);

}  // namespace hypo
