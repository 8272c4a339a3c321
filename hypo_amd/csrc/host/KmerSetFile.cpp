// KmerSetFile.cpp — see KmerSetFile.hpp.
#include "KmerSetFile.hpp"
#include <cerrno>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

static_assert(__BYTE_ORDER__ == __ORDER_LITTLE_ENDIAN__, "the file is little-endian and the values are written as they lie in memory");

namespace hypo {
namespace {
const char kMagic[8] = {'H', 'Y', 'P', 'O', 'K', 'S', 'E', 'T'};
constexpr uint32_t kVersion = 1;
struct Closer { void operator()(std::FILE* f) const { if (f) std::fclose(f); } };
using File = std::unique_ptr<std::FILE, Closer>;

bool put(std::FILE* f, const void* p, size_t n) { return !n || std::fwrite(p, 1, n, f) == n; }
bool get(std::FILE* f, void* p, size_t n) { return !n || std::fread(p, 1, n, f) == n; }

bool header_of(std::FILE* f, const std::string& path, KmerSetFileHeader& h, std::string& err) {
    char magic[8];
    if (!get(f, magic, 8) || !get(f, &h.version, 4) || !get(f, &h.k, 4) || !get(f, &h.n_keys, 8)) { err = path + ": short read in the header"; return false; }
    if (std::memcmp(magic, kMagic, 8) != 0) { err = path + ": bad magic: not a k-mer set file"; return false; }
    if (h.version != kVersion) { err = path + ": bad version " + std::to_string(h.version) + " (this build reads version " + std::to_string(kVersion) + ")"; return false; }
    return true;
}
}  // namespace

bool write_kmer_set_file(const std::string& path, uint32_t k, uint64_t n_keys, const KmerSetExportFn& next, uint64_t& bytes, std::string& err, int& rc,
                         uint64_t staging) {
    rc = 0;
    if (staging < 1 || staging > kKmerSetStaging) staging = kKmerSetStaging;
    const std::string tmp = path + ".tmp";
    File f(std::fopen(tmp.c_str(), "wb"));
    if (!f) { err = tmp + ": cannot be opened for writing: " + std::strerror(errno); return false; }
    auto fail = [&](const std::string& why) { f.reset(); std::remove(tmp.c_str()); err = why; return false; };
    // (a small set needs no large buffer; a call looks at `cap` slots of a table that is at most half full, often emptier)
    const uint64_t small = n_keys < ((uint64_t)1 << 18) ? (uint64_t)1 << 20 : 4 * n_keys;
    const uint64_t cap = small < staging ? small : staging;
    std::vector<uint64_t> keys(cap);
    std::vector<uint8_t> counts(cap + 8, 0);
    bool ok = put(f.get(), kMagic, 8) && put(f.get(), &kVersion, 4) && put(f.get(), &k, 4) && put(f.get(), &n_keys, 8);
    bytes = 24;
    uint64_t cursor = 0, digest = 0, sum = 0;
    while (ok && cursor != kKmerSetExportEnd) {
        uint64_t n = 0;
        if ((rc = next(&cursor, keys.data(), counts.data(), cap, &n, &digest)) != 0) return fail(path + ": the export of the set failed");
        if (n > cap) return fail(path + ": the export returned " + std::to_string(n) + " records for a buffer of " + std::to_string(cap));
        if (!n) continue;
        const size_t padded = (size_t)((n + 7) / 8 * 8);
        std::memset(counts.data() + n, 0, padded - (size_t)n);
        ok = put(f.get(), &n, 8) && put(f.get(), keys.data(), (size_t)n * 8) && put(f.get(), counts.data(), padded);
        bytes += 8 + n * 8 + padded;
        sum += n;
    }
    if (ok && sum != n_keys) return fail(path + ": the export returned " + std::to_string(sum) + " records, the set holds " + std::to_string(n_keys));
    const uint64_t zero = 0;
    ok = ok && put(f.get(), &zero, 8) && put(f.get(), &digest, 8);
    bytes += 16;
    std::FILE* raw = f.release();
    if (std::fclose(raw) != 0) ok = false;
    if (!ok) return fail(tmp + ": write error: " + std::strerror(errno));
    if (std::rename(tmp.c_str(), path.c_str()) != 0) return fail(tmp + ": cannot be moved to " + path + ": " + std::strerror(errno));
    return true;
}

bool read_kmer_set_header(const std::string& path, KmerSetFileHeader& h, std::string& err) {
    File f(std::fopen(path.c_str(), "rb"));
    if (!f) { err = path + ": cannot be opened: " + std::strerror(errno); return false; }
    if (!header_of(f.get(), path, h, err)) return false;
    // a record takes 9 bytes, a block 8 more, the end 16: a header that promises more records than the file can hold is refused
    // before anyone sizes a table by it
    if (std::fseek(f.get(), 0, SEEK_END) != 0) { err = path + ": cannot be measured: " + std::strerror(errno); return false; }
    const uint64_t size = (uint64_t)std::ftell(f.get());
    const uint64_t room = size >= 24 + 16 + 8 ? (size - 24 - 16 - 8) / 9 : 0;
    if (h.n_keys > room) {
        err = path + ": short read ahead: n_keys = " + std::to_string(h.n_keys) + " records need more than the file's " + std::to_string(size) + " bytes";
        return false;
    }
    return true;
}

bool read_kmer_set_file(const std::string& path, const KmerSetBlockFn& block, KmerSetFileHeader& h, uint64_t& digest, std::string& err, int& rc,
                        uint64_t staging) {
    rc = 0;
    if (staging < 1 || staging > kKmerSetStaging) staging = kKmerSetStaging;
    File f(std::fopen(path.c_str(), "rb"));
    if (!f) { err = path + ": cannot be opened: " + std::strerror(errno); return false; }
    if (!header_of(f.get(), path, h, err)) return false;
    auto fail = [&](const std::string& why) { err = path + ": " + why; return false; };
    std::vector<uint64_t> keys;
    std::vector<uint8_t> counts;
    uint64_t sum = 0;
    for (uint64_t b = 0;; ++b) {
        uint64_t n = 0;
        const std::string where = "block " + std::to_string(b);
        if (!get(f.get(), &n, 8)) return fail("short read at the length of " + where);
        if (!n) break;
        if (n > h.n_keys - sum) return fail(where + " of " + std::to_string(n) + " records would pass n_keys = " + std::to_string(h.n_keys));
        // the keys of a block lie in front of its counts: a block larger than the staging buffer is read piece by piece from both places
        const long keys_at = std::ftell(f.get());
        if (keys_at < 0) return fail("ftell failed");
        const uint64_t piece_max = n < staging ? n : staging;
        if (keys.size() < piece_max) { keys.resize((size_t)piece_max); counts.resize((size_t)piece_max); }
        for (uint64_t at = 0; at < n; at += piece_max) {
            const uint64_t m = n - at < piece_max ? n - at : piece_max;
            if (n > piece_max && std::fseek(f.get(), keys_at + (long)(at * 8), SEEK_SET) != 0) return fail("short read in the keys of " + where);
            if (!get(f.get(), keys.data(), (size_t)m * 8)) return fail("short read in the keys of " + where);
            if (n > piece_max && std::fseek(f.get(), keys_at + (long)(n * 8 + at), SEEK_SET) != 0) return fail("short read in the counts of " + where);
            if (!get(f.get(), counts.data(), (size_t)m)) return fail("short read in the counts of " + where);
            if ((rc = block(keys.data(), counts.data(), m)) != 0) return fail("records " + std::to_string(sum + at) + " to " + std::to_string(sum + at + m) + " (" + where + ") were refused");
        }
        uint8_t pad[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const size_t n_pad = (size_t)((8 - n % 8) % 8);
        if (!get(f.get(), pad, n_pad)) return fail("short read in the padding of " + where);
        for (size_t i = 0; i < n_pad; ++i) if (pad[i]) return fail("non-zero padding behind " + where);
        sum += n;
    }
    if (sum != h.n_keys) return fail("the blocks hold " + std::to_string(sum) + " records, below n_keys = " + std::to_string(h.n_keys));
    if (!get(f.get(), &digest, 8)) return fail("short read at the digest");
    if (std::fgetc(f.get()) != EOF) return fail("bytes after the digest");
    return true;
}

}  // namespace hypo
