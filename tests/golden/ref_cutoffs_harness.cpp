// ref_cutoffs_harness.cpp — C entry point around the REAL suk::SolidKmers::find_cutoffs (external/suk/src/SolidKmers.cpp:258-363),
// compiled from the reference's sources where they lie by tests/golden/make_solid_cutoffs_golden.py (the recipe of
// oracle/Makefile's libhyporef_scan.so: -ffunction-sections, --gc-sections, -z defs; SolidKmers::initialise and everything else
// that would need KMC is dropped, not stubbed).  TEST INFRASTRUCTURE ONLY: it generates tests/golden/solid_cutoffs.json.gz.
// The private member function is reached through explicit template instantiation, which the language exempts from access
// checks; the reference headers are included unmodified.
#include <cstdint>
#include <memory>
#include <vector>
#include "suk/SolidKmers.hpp"

namespace {
template <class Tag, typename Tag::type M> struct Rob { friend typename Tag::type get(Tag) { return M; } };
struct CutoffsTag { typedef suk::CutOffs (suk::SolidKmers::*type)(const std::vector<size_t>&); friend type get(CutoffsTag); };
template struct Rob<CutoffsTag, &suk::SolidKmers::find_cutoffs>;
}  // namespace

// hist[0 .. n_bins) -> out = {err, mean, lower, upper}.  The caller passes only histograms with a maximum after the error
// threshold (the reference leaves the mean unset otherwise).
extern "C" __attribute__((visibility("default"))) int hyporef_find_cutoffs(const uint64_t* hist, uint32_t n_bins, uint32_t* out) {
    auto sk = std::make_unique<suk::SolidKmers>(1);
    std::vector<size_t> h(hist, hist + n_bins);
    const suk::CutOffs c = ((*sk).*get(CutoffsTag()))(h);
    out[0] = c.err; out[1] = c.mean; out[2] = c.lower; out[3] = c.upper;
    return 0;
}
