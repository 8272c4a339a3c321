// kset_file_reader_main.cpp — TEST PROGRAM (tests/test_kset_file_reader_cpu.py): the reader and the writer of
// hypo_amd/csrc/host/KmerSetFile.cpp without a device, built with -fsanitize=address,undefined.
//   kset_file_reader_main read <file> [staging]     every block through a callback that sums the records' digests
//       accepted: prints "ok k=<k> n_keys=<n> records=<fed> pieces=<calls> largest=<records> digest=<hex> sum=<hex>", exit 0
//       refused:  prints "refused: <message>", exit 3
//   kset_file_reader_main header <file>             the header alone: "ok k=<k> n_keys=<n>", or "refused: <message>" and exit 3
//   kset_file_reader_main copy <file> <out> [cap]   reads <file> into memory and writes it to <out> through the writer, with an
//       export callback that hands the records out `cap` slots at a time (every other slot empty), exit 0 / "refused: ..." and 3
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../hypo_amd/csrc/host/KmerSetFile.hpp"

static uint64_t mix64(uint64_t x) {
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return x;
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const std::string mode = argv[1], path = argv[2];
    hypo::KmerSetFileHeader h;
    std::string err;
    if (mode == "header") {
        if (!hypo::read_kmer_set_header(path, h, err)) { std::printf("refused: %s\n", err.c_str()); return 3; }
        std::printf("ok k=%u n_keys=%llu\n", h.k, (unsigned long long)h.n_keys);
        return 0;
    }
    int rc = 0;
    uint64_t in_file = 0, sum = 0, fed = 0, pieces = 0, largest = 0;
    std::vector<uint64_t> keys;
    std::vector<uint8_t> counts;
    const bool keep = mode == "copy";
    const uint64_t staging = mode == "read" && argc > 3 ? std::strtoull(argv[3], nullptr, 10) : hypo::kKmerSetStaging;
    const bool ok = hypo::read_kmer_set_file(path, [&](const uint64_t* k, const uint8_t* c, uint64_t n) {
        for (uint64_t i = 0; i < n; ++i) sum += mix64(k[i]) + (uint64_t)c[i] * 0x9e3779b97f4a7c15ull;
        if (keep) { keys.insert(keys.end(), k, k + n); counts.insert(counts.end(), c, c + n); }
        fed += n; ++pieces; if (n > largest) largest = n;
        return 0;
    }, h, in_file, err, rc, staging);
    if (!ok) { std::printf("refused: %s\n", err.c_str()); return 3; }
    if (mode == "read") {
        std::printf("ok k=%u n_keys=%llu records=%llu pieces=%llu largest=%llu digest=%016llx sum=%016llx\n", h.k, (unsigned long long)h.n_keys,
                    (unsigned long long)fed, (unsigned long long)pieces, (unsigned long long)largest, (unsigned long long)in_file, (unsigned long long)sum);
        return 0;
    }
    if (argc < 4) return 2;
    const uint64_t cap = argc > 4 ? std::strtoull(argv[4], nullptr, 10) : 7;
    // a table of 2 n "slots", the records in the even ones: a call looks at `cap` slots, as hypo_gpu_kset_export does
    const uint64_t slots = 2 * (uint64_t)keys.size();
    uint64_t bytes = 0;
    const bool wrote = hypo::write_kmer_set_file(argv[3], h.k, h.n_keys, [&](uint64_t* cursor, uint64_t* k, uint8_t* c, uint64_t room, uint64_t* n_out, uint64_t* digest) {
        const uint64_t take = room < cap ? room : cap;
        uint64_t s = *cursor, n = 0;
        for (; s < slots && s < *cursor + take; ++s)
            if (s % 2 == 0) { k[n] = keys[s / 2]; c[n] = counts[s / 2]; *digest += mix64(k[n]) + (uint64_t)c[n] * 0x9e3779b97f4a7c15ull; ++n; }
        *n_out = n;
        *cursor = s >= slots ? hypo::kKmerSetExportEnd : s;
        return 0;
    }, bytes, err, rc);
    if (!wrote) { std::printf("refused: %s\n", err.c_str()); return 3; }
    std::printf("ok bytes=%llu\n", (unsigned long long)bytes);
    return 0;
}
