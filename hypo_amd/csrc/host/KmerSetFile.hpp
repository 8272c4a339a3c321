// KmerSetFile.hpp — the k-mer set of the reads as a file (hypo --qv-save / --qv-load; DESIGN.md "k-mer set file").  Plain host
// code: neither the writer nor the reader knows of the device, they move records between a file and a callback.
//
// The file, little-endian:
//   header, 24 bytes   "HYPOKSET", u32 version = 1, u32 k, u64 n_keys
//   blocks             u64 n (n >= 1), n keys as u64, n count bytes, zero bytes up to the next multiple of 8
//   end                u64 0, u64 digest, then the end of the file
// A key is a canonical code (min(fwd, rc), A0 C1 G2 T3, MSB-first, below 4^k), a count byte 1..255 (1 from a set that does not
// count).  The blocks' n add up to n_keys.  digest = the sum over all records of mix64(key) + count * 0x9e3779b97f4a7c15 (mod 2^64;
// mix64: the finaliser of MurmurHash3, include/hypo_gpu.h), so it does not depend on the order of the records.
#pragma once
#include <cstdint>
#include <functional>
#include <string>

namespace hypo {

struct KmerSetFileHeader { uint32_t version = 0, k = 0; uint64_t n_keys = 0; };
constexpr uint64_t kKmerSetStaging = (uint64_t)1 << 24;     // most records the writer asks for, and the reader hands on, at a time
constexpr uint64_t kKmerSetExportEnd = ~(uint64_t)0;       // HYPO_KSET_EXPORT_END

// hypo_gpu_kset_export: (cursor, keys, counts, cap, n_out, digest) -> 0 or an error code
using KmerSetExportFn = std::function<int(uint64_t*, uint64_t*, uint8_t*, uint64_t, uint64_t*, uint64_t*)>;
// one piece of a block: (keys, counts, n) -> 0 or an error code (hypo --qv-load: hypo_gpu_kset_import)
using KmerSetBlockFn = std::function<int(const uint64_t*, const uint8_t*, uint64_t)>;

// Writes <path>.tmp from ONE export sequence (calls of at most `staging` <= kKmerSetStaging records, one block per call that
// returned any), checks that the calls returned n_keys records, writes the end and renames the file to `path`: the file is complete
// the moment it has its name.  false: `err` names the file and the cause (`rc` = the callback's code when it was the cause, else
// 0), and <path>.tmp is gone.  bytes: the size of the file.
bool write_kmer_set_file(const std::string& path, uint32_t k, uint64_t n_keys, const KmerSetExportFn& next, uint64_t& bytes, std::string& err, int& rc,
                         uint64_t staging = kKmerSetStaging);

// The header alone, for a caller that sizes a table by n_keys before it reads the blocks.  false: the file cannot be opened, is
// shorter than a header, has another magic or version, or is too short for n_keys records (9 bytes each, one block, the end).
bool read_kmer_set_header(const std::string& path, KmerSetFileHeader& h, std::string& err);

// The whole file: every block goes to `block` in pieces of at most `staging` records.  Refused, with `err` naming the file and the
// cause: a bad magic or version, a short read anywhere, padding that is not zero, an empty block, a block that would pass n_keys, a
// sum below n_keys at the end marker, bytes after the digest, and a callback that answers other than 0 (`rc` = its code, else 0).
// digest: the one the file states; the caller compares it with what it made of the records.
bool read_kmer_set_file(const std::string& path, const KmerSetBlockFn& block, KmerSetFileHeader& h, uint64_t& digest, std::string& err, int& rc,
                        uint64_t staging = kKmerSetStaging);

}  // namespace hypo
