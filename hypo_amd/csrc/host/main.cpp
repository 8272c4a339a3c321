// main.cpp — command line of the MI355X build: the reference's flags and defaults (src/main.cpp:46-67,100-113,
// 124-358) plus the opt-in flags --device / --gpus / --devices.  usage() keeps the reference's layout, the wording is this build's own.
#include <getopt.h>
#include <unistd.h>
#include <malloc.h>
#include <sys/stat.h>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include "Hypo.hpp"

namespace {

const struct option long_options[] = {
    {"reads-short", required_argument, nullptr, 'r'}, {"draft", required_argument, nullptr, 'd'},
    {"size-ref", required_argument, nullptr, 's'}, {"coverage-short", required_argument, nullptr, 'c'},
    {"bam-sr", required_argument, nullptr, 'b'}, {"bam-lr", required_argument, nullptr, 'B'},
    {"output", required_argument, nullptr, 'o'}, {"threads", required_argument, nullptr, 't'},
    {"processing-size", required_argument, nullptr, 'p'}, {"kind-sr", required_argument, nullptr, 'k'},
    {"match-sr", required_argument, nullptr, 'm'}, {"mismatch-sr", required_argument, nullptr, 'x'},
    {"gap-sr", required_argument, nullptr, 'g'}, {"match-lr", required_argument, nullptr, 'M'},
    {"mismatch-lr", required_argument, nullptr, 'X'}, {"gap-lr", required_argument, nullptr, 'G'},
    {"qual-map-th", required_argument, nullptr, 'q'}, {"ned-th", required_argument, nullptr, 'n'},
    {"intermed", no_argument, nullptr, 'i'}, {"help", no_argument, nullptr, 'h'},
    {"device", required_argument, nullptr, 1000}, {"gpus", required_argument, nullptr, 1001},
    {"devices", required_argument, nullptr, 1002}, {"native-klov", no_argument, nullptr, 1003},
    {"ccs-windows", no_argument, nullptr, 1004}, {"host-arms", no_argument, nullptr, 1005}, {"require-device", no_argument, nullptr, 1006},
    {"vcf", required_argument, nullptr, 1007}, {"qv", required_argument, nullptr, 1008}, {"qv-k", required_argument, nullptr, 1009},
    {"qv-mem", required_argument, nullptr, 1010}, {"kmer-guard", no_argument, nullptr, 1011},
    {"guard-records", no_argument, nullptr, 1012}, {"guard-records-max", required_argument, nullptr, 1013},
    {"qv-bed", required_argument, nullptr, 1014}, {"qv-spectra", required_argument, nullptr, 1015},
    {"qv-reliable-min", required_argument, nullptr, 1016}, {"qv-min-count", required_argument, nullptr, 1017},
    {"kmer-fix", required_argument, nullptr, 1018}, {"kmer-bridge", required_argument, nullptr, 1019},
    {"kmer-bridge-max", required_argument, nullptr, 1020}, {"kmer-bridge-slack", required_argument, nullptr, 1021},
    {"kmer-bridge-vote", required_argument, nullptr, 1022}, {"qv-save", required_argument, nullptr, 1023},
    {"qv-load", required_argument, nullptr, 1024}, {"qv-cn", required_argument, nullptr, 1025},
    {"qv-cn-bin", required_argument, nullptr, 1026}, {"qv-cn-unit", required_argument, nullptr, 1027}, {nullptr, 0, nullptr, 0}};

// Same layout as the reference's usage() (src/main.cpp:363-430): "Usage: hypo <args>", the mandatory block, the optional
// block, every flag as "-x, --long <type>" followed by what it does and its default.  The wording is this build's own.
struct HelpEntry { const char* flag; const char* what; const char* dflt; };
void usage() {
    static const HelpEntry mandatory[] = {
        {"-r, --reads-short <str>", "Short reads (fasta/fastq, plain or compressed), or @file holding one file name per line. The solid k-mers are counted from them on the device (k = 5..17); with -i a stored aux/solid_kmers.bvsd is used instead.", nullptr},
        {"-d, --draft <str>", "Draft contigs to polish (fasta/fastq, plain or compressed).", nullptr},
        {"-b, --bam-sr <str>", "Short reads aligned to the draft (bam, or sam plain/gzip; CIGAR required), sorted by coordinate.", nullptr},
        {"-c, --coverage-short <int>", "Approximate mean coverage of the short reads.", nullptr},
        {"-s, --size-ref <str>", "Approximate genome size: a number, optionally followed by k/m/g (10m, 2.3g). It fixes the solid k-mer length.", nullptr}};
    static const HelpEntry optional[] = {
        {"-B, --bam-lr <str>", "Long reads aligned to the draft (bam/sam with CIGAR).", "short-read polishing only"},
        {"-o, --output <str>", "Output file.", "hypo_<draft_file_name>.fasta in the working directory"},
        {"-t, --threads <int>", "Host threads.", "1"},
        {"-p, --processing-size <int>", "Contigs per batch; fewer contigs per batch need less memory.", "all contigs of the draft"},
        {"-k, --kind-sr <str>", "Kind of short reads: sr (Illumina-like) or ccs (HiFi). Accepted and, as in the reference (src/main.cpp:312), without effect.", "sr"},
        {"-m, --match-sr <int>", "Match score, short reads.", "5"},
        {"-x, --mismatch-sr <int>", "Mismatch score, short reads.", "-4"},
        {"-g, --gap-sr <int>", "Gap penalty, short reads (negative).", "-8"},
        {"-M, --match-lr <int>", "Match score, long reads.", "3"},
        {"-X, --mismatch-lr <int>", "Mismatch score, long reads.", "-5"},
        {"-G, --gap-lr <int>", "Gap penalty, long reads (negative).", "-4"},
        {"-n, --ned-th <int>", "Largest normalised edit distance (in %) of a long arm that may enter a window.", "20"},
        {"-q, --qual-map-th <int>", "Reads mapped with a quality below this are ignored.", "2"},
        {"-i, --intermed", "Keep and reuse intermediate files: the solid k-mer set is stored in aux/solid_kmers.bvsd (and stage 1 in aux/stage.txt) and loaded by later runs.", nullptr},
        {"    --device <int>", "[MI355X build] HIP device to run on.", "0"},
        {"    --gpus <int>", "[MI355X build] Use devices 0..N-1, one context each: the contigs of a batch are dealt out to them (a contig larger than its share is cut into coordinate ranges), every context votes, cuts arms and polishes its own resident windows; windows that exist as host objects are sharded with an RCCL gather.", "1"},
        {"    --devices <list>", "[MI355X build] Comma-separated HIP device ids instead of --device / --gpus.", nullptr},
        {"    --native-klov", "[MI355X build] Choose the end row of prefix arms like the AVX2 / SSE4.1 alignment engine of a -march=native build of the reference does (the default follows the scalar engine of the reference's default build; the two differ on noisy prefix arms).", "off"},
        {"    --ccs-windows", "[MI355X build] Cut windows with the sizes -k ccs was meant to select (ideal length 500, search threshold 400; the reference parses -k but never applies it).", "off"},
        {"    --host-arms", "[MI355X build] Cut the short reads into arms on the host (the reference's loops) instead of on the device.", "off"},
        {"    --require-device", "[MI355X build] Exit with an error, instead of an Info line and the host loops, when a stage the device should run (support votes, arm selection) cannot run there (also: HYPO_REQUIRE_DEVICE=1).", "off"},
        {"    --vcf <str>", "[MI355X build] Also write every change the polishing made to the draft as a VCF 4.2 file (REF = draft bases, ALT = polished bases; the alignment of each replaced stretch is computed on the device).", "no VCF"},
        {"    --qv <str>", "[MI355X build] Also write the reference-free k-mer QV of every draft contig and of its polished text as a tab-separated file: the canonical k-mers of the short reads (-r) are kept as an exact set on the device, and a k-mer of a contig that is not among them counts as an error (Merqury's definition). The reads are parsed once for this and the solid k-mers; a run that starts from stage 1 (-i) parses them for the QV alone.", "no QV"},
        {"    --qv-k <int>", "[MI355X build] k-mer length of --qv, 12 to 31.", "21"},
        {"    --qv-mem <GiB>", "[MI355X build] Largest table the k-mer set of --qv may grow to; a read set that needs more ends the run before any contig is polished.", "half of the device's free memory"},
        {"    --qv-save <str>", "[MI355X build] Also write the k-mer set of the short reads to this file when the last read is in, before any contig is polished: every k-mer with the number of times the reads contain it (up to 255), whatever --qv-min-count says, so that the file serves every flag of a later run. The set is built and stored even when no other flag asks for it, and counts as under --qv-min-count (one more byte a slot under --qv-mem); every other output is what it is without the flag. The file is written under <file>.tmp and complete the moment it has its name; a run that fails later keeps it.", "the set is not stored"},
        {"    --qv-load <str>", "[MI355X build] Fill the k-mer set from a file of --qv-save instead of from the short reads: the reads are not parsed for it (a run that starts from stage 1 opens none), and every output file is byte for byte that of the run that built the set. The file's k must be --qv-k; a file that is damaged, or whose records do not add up to its digest, ends the run before any output is opened. Needs a flag that asks the set (--qv, --qv-bed, --qv-spectra, --kmer-guard, --kmer-fix, --kmer-bridge); not together with --qv-save.", "the set is built from the reads"},
        {"    --kmer-guard", "[MI355X build] Keep only the edits the k-mers of the short reads support: edits closer than k - 1 draft bases form a cluster, and a cluster that puts more k-mers no read contains into the contig than it removes is left out of the output (its VCF records get FILTER kmer instead of PASS; the polished columns of --qv describe the guarded text). Uses the k-mer set of --qv (--qv-k, --qv-mem) with or without --qv and --vcf.", "off"},
        {"    --guard-records", "[MI355X build] Implies --kmer-guard, and decides a cluster of 2 to --guard-records-max edits record by record: of all subsets of the cluster's records the one whose text lacks the fewest k-mers of the reads is kept (among equals the one with the most records), the other records get FILTER kmer. A single bad edit then no longer costs its neighbours. Larger clusters are accepted or rejected whole, as with --kmer-guard.", "off"},
        {"    --guard-records-max <int>", "[MI355X build] Most records of a cluster --guard-records still decides one by one, 2 to 12 (a cluster of n records has 2^n subsets). Without --guard-records it has no effect.", "8"},
        {"    --qv-bed <str>", "[MI355X build] Also write where the polished text (with --kmer-guard the guarded text) still disagrees with the short reads, as a BED file: a base is covered when a k-mer that no read contains (the missing k-mers of --qv) lies over it, every maximal run of covered bases of a contig is one line, contig, start, end (0-based, end exclusive) and the number of missing k-mers inside. Per contig the fourth column adds up to polished_missing of --qv. Uses the k-mer set of --qv (--qv-k, --qv-mem) with or without --qv, --vcf and --kmer-guard; the intervals are found on the device.", "no BED"},
        {"    --qv-spectra <str>", "[MI355X build] Also write the copy-number spectrum and the k-mer completeness of the draft and of the polished text (with --kmer-guard the guarded text) as a tab-separated file: the k-mer set of --qv also counts how often the short reads contain every k-mer, and per read multiplicity 1 to 255 the file tells how many distinct read k-mers the text contains 0, 1, 2, 3 and 4 or more times (Merqury's spectra-cn: a collapsed or duplicated stretch moves k-mers between the columns). Completeness is the share of the reliable read k-mers (seen at least --qv-reliable-min times) that the text contains; asm_only_windows are the text's k-mers no read contains, polished_missing of --qv. Uses --qv-k and --qv-mem, with or without --qv, --qv-bed, --vcf and --kmer-guard; counted and compared on the device.", "no spectra"},
        {"    --qv-reliable-min <int>", "[MI355X build] Least number of times the short reads must contain a k-mer for it to count as reliable in the completeness of --qv-spectra, 1 to 255.", "the valley of the read k-mer histogram: the smallest multiplicity from 2 on at which it stops falling"},
        {"    --qv-min-count <int|valley>", "[MI355X build] Count a read k-mer only when the short reads contain it at least this often, 1 to 255, or `valley`: the valley of the read k-mer histogram, the default of --qv-reliable-min. A k-mer seen fewer times is mostly a sequencing error and then counts as missing wherever the reads are asked: in the missing columns and QVs of --qv, the intervals of --qv-bed, and the decisions of --kmer-guard and --guard-records. Needs at least one of those four; 1 is the run without the flag. The k-mer set then counts as for --qv-spectra (one more byte a slot under --qv-mem), whose file does not change.", "1: a k-mer seen once is present"},
        {"    --kmer-fix <str>", "[MI355X build] Make one pass of single-base fixes over the text that would otherwise be written (with --kmer-guard the guarded text), where the k-mers of the short reads pin an isolated error down: a stretch of at most 2k - 1 bases in which every k-mer is one no read contains, at least k - 1 bases from the next such stretch and not at a contig end, is tried with every substitution, deletion and insertion of one base at the positions all its k-mers share, and fixed when exactly one of the edited texts lacks no k-mer of the reads; two such texts (a heterozygous base, a read error) leave it alone. The file lists the fixes, tab-separated: contig, pos (0-based, in the text before the fixes), kind (sub, del, ins), ref, alt, and the missing k-mers the fix removes. --qv, --qv-bed and --qv-spectra then describe the fixed text; --vcf still describes the text before the fixes. Uses the k-mer set of --qv (--qv-k, --qv-mem, --qv-min-count) with or without the other flags; the edits are tried on the device.", "no fixes"},
        {"    --kmer-bridge <str>", "[MI355X build] Make one pass of local reassembly over the text that would otherwise be written (after --kmer-guard and --kmer-fix), where the k-mers of the short reads spell exactly one other text: a stretch under k-mers no read contains, at least 2 bases from the next such stretch and not at a contig end, lies between two k-mers the reads do contain, one base in front of it and one behind it. When those two anchors are at most --kmer-bridge-max bases apart, the k-mers of the reads are walked as a de Bruijn graph from the left anchor to the right one, letting the stretch grow or shrink by up to --kmer-bridge-slack bases, and when exactly one walk arrives its text replaces the stretch; several walks (a heterozygous site, a repeat) or a search that gives up leave it alone. This reaches what --kmer-fix leaves behind: length errors of two or more bases in homopolymers and short tandem repeats, substitutions closer than k, an indel next to a substitution. The file lists the bridges, tab-separated: contig, pos (0-based, in the text before this pass), ref, alt (`.` when empty), the missing k-mers the bridge removes, and the steps of the search. --qv, --qv-bed and --qv-spectra then describe the bridged text; --vcf still describes the text before the fixes and bridges. Uses the k-mer set of --qv (--qv-k, --qv-mem, --qv-min-count) with or without the other flags; the graph is walked on the device.", "no bridges"},
        {"    --kmer-bridge-max <int>", "[MI355X build] Largest distance of the two anchors --kmer-bridge still tries, 2 to 192 bases. Needs --kmer-bridge.", "64"},
        {"    --kmer-bridge-slack <int>", "[MI355X build] Most bases a bridge of --kmer-bridge may add to or remove from the stretch it replaces, 0 to 64. Needs --kmer-bridge.", "8"},
        {"    --kmer-bridge-vote <int>", "[MI355X build] Settle the stretches --kmer-bridge leaves as ambiguous by read count: such a stretch is searched again for up to 4 walks, each with its support, the smallest number of times the short reads contain a k-mer of the walk, and when the best walk's support is at least this many times the second best's, 2 to 255, its text replaces the stretch (a read error seen once against an allele seen 30 times). Walks of similar support (a heterozygous site, a repeat), more than 4 walks or a search that gives up leave it alone. The file of --kmer-bridge gains two columns: the walks found (1 for a bridge that needed no vote) and the two supports as best/second (`.` without a vote). The k-mer set then counts as for --qv-min-count (one more byte a slot under --qv-mem), with or without --qv-min-count. Needs --kmer-bridge.", "no vote"},
        {"    --qv-cn <str>", "[MI355X build] Also write where the copy number of the text that is written (after --kmer-guard, --kmer-fix and --kmer-bridge) disagrees with the short reads, as a tab-separated file: a collapsed repeat, a collapsed pair of haplotypes or a falsely duplicated stretch loses no k-mer, so --qv and --qv-bed do not see it. The k-mer set of --qv also counts how often the short reads contain every k-mer, and once the last contig is written, how often the whole text does. Per bin of --qv-cn-bin k-mer starts of every contig the file tells the k-mers, the missing ones (those of --qv), the rated ones (present, neither count at its cap of 255), how many of those the reads contain at least 1.5 times as often as the text's copies at --qv-cn-unit reads each ask for (over) and at most 0.75 times as often (under), and the median read count; a bin is called collapsed when more than half of its rated k-mers are over, duplicated when more than half are under. The two factors are the rounded geometric midpoints between one copy and two, and between a half and one; the raw columns are there to apply others. Every contig's text is kept until the last one is written (one byte a base of host memory). Uses --qv-k, --qv-mem, --qv-min-count, --qv-save and --qv-load, with or without the other flags; the k-mer set counts as for --qv-spectra (one or two more bytes a slot under --qv-mem); counted and compared on the device.", "no copy-number file"},
        {"    --qv-cn-bin <int>", "[MI355X build] k-mer starts per line of --qv-cn, 32 to 65536. Needs --qv-cn.", "1024"},
        {"    --qv-cn-unit <int>", "[MI355X build] How often the short reads contain a k-mer the genome holds once, 1 to 255: the read count --qv-cn takes for one copy. Needs --qv-cn.", "the peak of the read k-mer histogram: the most frequent multiplicity from its valley on (a run whose histogram has none ends with an error that asks for this flag)"},
        {"-h, --help", "Print the usage.", nullptr}};
    std::printf("\n Usage: hypo <args>\n\n ** Mandatory args:\n");
    for (const auto& e : mandatory) std::printf("\t%s\n\t%s\n\n", e.flag, e.what);
    std::printf("\n ** Optional args:\n");
    for (const auto& e : optional) {
        std::printf("\t%s\n\t%s\n", e.flag, e.what);
        if (e.dflt) std::printf("\t[Default] %s.\n", e.dflt);
        std::printf("\n");
    }
}

bool file_exists(const std::string& p) { struct stat st; return stat(p.c_str(), &st) == 0; }

// src/main.cpp:490-528: smallest odd k with 4^k >= genome size
unsigned get_kmer_len(const std::string& given, uint64_t* size_out = nullptr) {
    size_t ind = 0;
    const float val = std::stof(given, &ind);
    unsigned power = 0;
    if (ind >= given.size()) {
        if (std::floor(val) != std::ceil(val)) { std::fprintf(stderr, "[Hypo::Utils] Error: Wrong format for genome-size: Genome-size with no units (K,M,G etc,) should be absolute number!\n"); std::exit(1); }
    } else {
        switch (std::toupper(given[ind])) {
            case 'K': power = 10; break; case 'M': power = 20; break; case 'G': power = 30; break; case 'T': power = 40; break;
            default: std::fprintf(stderr, "[Hypo::Utils] Error: Wrong format for genome-size: Allowed units for Genome-size are K (10^3),M (10^6),G (10^9),T (10^12)!\n"); std::exit(1);
        }
    }
    if (size_out) *size_out = (uint64_t)std::min(std::ldexp((double)val, (int)power), 9e18);
    unsigned k = (unsigned)((double)power + std::ceil(std::log2(val)));
    k = (unsigned)std::ceil(k / 2);                 // integer division first, as in the reference
    if (k % 2 == 0) ++k;
    std::fprintf(stdout, "[Hypo::Utils] Info: Value of K chosen for the given genome size (%s): %u\n", given.c_str(), k);
    return k;
}

}  // namespace

int main(int argc, char** argv) {
    // The host stages allocate millions of small objects (alignments, arms) from all threads.  glibc grows a thread arena in
    // small mprotect steps and trims it eagerly; with > 32 threads those system calls serialise on the address-space lock
    // (measured: -t 64 took 2.1 s instead of 1.05 s on the 5 Mbp set).  Grow in 64 MB steps, give memory back late.
    // The OpenMP workers must sleep between parallel regions: the run alternates short parallel phases with serial stretches,
    // device calls and helper threads (record reader, releasers, the HIP runtime's own), and libgomp's default lets idle workers
    // spin — measured on the 100 x 1 Mbp set, -t 64: 8.98 s spinning, 4.77 s sleeping (profiles/diag/r03_c3_threads.sh).  libgomp
    // reads the policy when it is loaded, i.e. before main(): set it and start over once.
    // HYPO_NO_REEXEC=1 (or an OMP_WAIT_POLICY of the caller's own) opts out; a traced process (debugger, strace, profilers that
    // attach) is never re-executed either — it would lose its tracer's state.
    auto traced = [] {
        std::ifstream st("/proc/self/status");
        std::string key; long v = 0;
        while (st >> key) { if (key == "TracerPid:") { st >> v; return v != 0; } st.ignore(4096, '\n'); }
        return false;
    };
    if (!getenv("OMP_WAIT_POLICY") && !getenv("HYPO_NO_REEXEC") && !traced()) {
        setenv("OMP_WAIT_POLICY", "passive", 1);
        setenv("HYPO_NO_REEXEC", "1", 1);
        execv("/proc/self/exe", argv);                          // (if this fails the run goes on with the default policy)
    }
    mallopt(M_TOP_PAD, 64 << 20);
    mallopt(M_TRIM_THRESHOLD, 1 << 30);
    hypo::InputFlags flags;
    bool is_sr = false, is_draft = false, is_size = false, is_cov = false, is_bamsr = false;
    std::string given_sz, kind = "sr";
    int opt;
    bool cn_opts = false;                                                  // --qv-cn-bin or --qv-cn-unit was given
    bool bridge_opts = false;                                              // --kmer-bridge-max or --kmer-bridge-slack was given
    auto int_in = [](const char* flag, const char* arg, long lo, long hi) {
        char* end = nullptr;
        const long v = std::strtol(arg, &end, 10);
        if (end == arg || *end || v < lo || v > hi) { std::fprintf(stderr, "[Hypo::] Error: Arg Error: %s must be between %ld and %ld %s!\n", flag, lo, hi, arg); std::exit(1); }
        return (uint32_t)v;
    };
    auto need_file = [](const char* what, const std::string& p) {
        if (!file_exists(p)) { std::fprintf(stderr, "[Hypo::] Error: File Error: %s file does not exist %s!\n", what, p.c_str()); std::exit(1); }
    };
    while ((opt = getopt_long(argc, argv, "r:d:s:c:b:B:o:t:p:k:m:x:g:M:X:G:q:n:ih", long_options, nullptr)) != -1) {
        switch (opt) {
            case 'r': {
                std::string in = optarg;
                if (!in.empty() && in[0] == '@') {
                    std::ifstream f(in.substr(1));
                    if (!f) { std::fprintf(stderr, "[Hypo::] Error: File Error: Reads file-list does not exist %s!\n", in.c_str()); std::exit(1); }
                    std::string name;
                    while (std::getline(f, name)) if (!name.empty()) { need_file("Reads", name); flags.sr_filenames.push_back(name); }
                } else { need_file("Reads", in); flags.sr_filenames.push_back(in); }
                is_sr = true; break;
            }
            case 'd': flags.draft_filename = optarg; need_file("Draft", flags.draft_filename); is_draft = true; break;
            case 's': given_sz = optarg; flags.k = std::max(2u, get_kmer_len(given_sz, &flags.genome_size)); is_size = true; break;
            case 'c': flags.cov = (uint32_t)std::atoi(optarg); if (flags.cov == 0) { std::fprintf(stderr, "[Hypo::] Error: Arg Error: Coverage should be a positive integer %s!\n", optarg); std::exit(1); } is_cov = true; break;
            case 'b': flags.sr_bam_filename = optarg; need_file("Short reads BAM", flags.sr_bam_filename); is_bamsr = true; break;
            case 'B': flags.lr_bam_filename = optarg; need_file("Long reads BAM", flags.lr_bam_filename); break;
            case 'o': flags.output_filename = optarg; break;
            case 't': flags.threads = (uint32_t)std::max(1, std::atoi(optarg)); break;
            case 'p': flags.processing_batch_size = (uint32_t)std::max(0, std::atoi(optarg)); break;
            case 'k': kind = optarg; break;                               // parsed, never applied (src/main.cpp:312)
            case 'm': flags.score_params.sr_match = (int8_t)std::atoi(optarg); break;
            case 'x': flags.score_params.sr_mismatch = (int8_t)std::atoi(optarg); break;
            case 'g': flags.score_params.sr_gap = (int8_t)std::atoi(optarg);
                      if (flags.score_params.sr_gap >= 0) { std::fprintf(stderr, "[Hypo::] Error: Arg Error: Gap penalty must be negative %s!\n", optarg); std::exit(1); } break;
            case 'M': flags.score_params.lr_match = (int8_t)std::atoi(optarg); break;
            case 'X': flags.score_params.lr_mismatch = (int8_t)std::atoi(optarg); break;
            case 'G': flags.score_params.lr_gap = (int8_t)std::atoi(optarg);
                      if (flags.score_params.lr_gap >= 0) { std::fprintf(stderr, "[Hypo::] Error: Arg Error: Gap penalty must be negative %s!\n", optarg); std::exit(1); } break;
            case 'q': flags.map_qual_th = (uint32_t)std::max(0, std::atoi(optarg)); break;
            case 'n': flags.norm_edit_th = (uint32_t)std::max(0, std::atoi(optarg)); break;
            case 'i': flags.intermed = true; break;
            case 1000: flags.device = std::atoi(optarg); break;
            case 1001: flags.gpus = std::max(1, std::atoi(optarg)); break;
            case 1003: flags.native_klov = true; break;
            case 1004: flags.ccs_windows = true; break;
            case 1005: flags.host_arms = true; break;
            case 1006: flags.require_device = true; break;
            case 1007: flags.vcf_filename = optarg; break;
            case 1008: flags.qv_filename = optarg; break;
            case 1009: {
                const int v = std::atoi(optarg);
                if (v < 12 || v > 31) { std::fprintf(stderr, "[Hypo::] Error: Arg Error: --qv-k must be between 12 and 31 (the k-mer set keeps 2k-bit codes in 64-bit slots) %s!\n", optarg); std::exit(1); }
                flags.qv_k = (uint32_t)v; break;
            }
            case 1010: flags.qv_mem_gib = std::atof(optarg);
                       if (!(flags.qv_mem_gib > 0)) { std::fprintf(stderr, "[Hypo::] Error: Arg Error: --qv-mem must be a positive number of GiB %s!\n", optarg); std::exit(1); } break;
            case 1011: flags.kmer_guard = true; break;
            case 1012: flags.guard_records = flags.kmer_guard = true; break;
            case 1013: {
                char* end = nullptr;
                const long v = std::strtol(optarg, &end, 10);
                if (end == optarg || *end || v < 2 || v > 12) { std::fprintf(stderr, "[Hypo::] Error: Arg Error: --guard-records-max must be between 2 and 12 (a cluster of n records has 2^n subsets) %s!\n", optarg); std::exit(1); }
                flags.guard_records_max = (uint32_t)v; break;
            }
            case 1014: flags.qv_bed_filename = optarg; break;
            case 1015: flags.qv_spectra_filename = optarg; break;
            case 1016: {
                char* end = nullptr;
                const long v = std::strtol(optarg, &end, 10);
                if (end == optarg || *end || v < 1 || v > 255) { std::fprintf(stderr, "[Hypo::] Error: Arg Error: --qv-reliable-min must be between 1 and 255 (the k-mer set counts up to 255) %s!\n", optarg); std::exit(1); }
                flags.qv_reliable_min = (uint32_t)v; break;
            }
            case 1017: {
                char* end = nullptr;
                const long v = std::strtol(optarg, &end, 10);
                const bool valley = std::string(optarg) == "valley";
                if (!valley && (end == optarg || *end || v < 1 || v > 255)) { std::fprintf(stderr, "[Hypo::] Error: Arg Error: --qv-min-count must be between 1 and 255 (the k-mer set counts up to 255) or `valley` %s!\n", optarg); std::exit(1); }
                flags.qv_min_count = valley ? 0 : (uint32_t)v; break;                // (0: the valley, found when the reads are in)
            }
            case 1018: flags.kmer_fix_filename = optarg; break;
            case 1019: flags.kmer_bridge_filename = optarg; break;
            case 1020: flags.kmer_bridge_max = int_in("--kmer-bridge-max", optarg, 2, 192); bridge_opts = true; break;
            case 1021: flags.kmer_bridge_slack = int_in("--kmer-bridge-slack", optarg, 0, 64); bridge_opts = true; break;
            case 1022: flags.kmer_bridge_vote = int_in("--kmer-bridge-vote", optarg, 2, 255); break;
            case 1023: flags.qv_save_filename = optarg; break;
            case 1024: flags.qv_load_filename = optarg; break;
            case 1025: flags.qv_cn_filename = optarg; break;
            case 1026: flags.qv_cn_bin = int_in("--qv-cn-bin", optarg, 32, 65536); cn_opts = true; break;
            case 1027: flags.qv_cn_unit = int_in("--qv-cn-unit", optarg, 1, 255); cn_opts = true; break;
            case 1002: {
                flags.devices.clear();
                for (const char* c = optarg; *c;) { flags.devices.push_back(std::atoi(c)); while (*c && *c != ',') ++c; if (*c == ',') ++c; }
                break;
            }
            default: usage(); return 0;                                    // -h and unknown options alike (src/main.cpp:302-304)
        }
    }
    if (cn_opts && flags.qv_cn_filename.empty()) {
        std::fprintf(stderr, "[Hypo::] Error: Arg Error: --qv-cn-bin and --qv-cn-unit set how --qv-cn reads the text: they need --qv-cn!\n");
        std::exit(1);
    }
    if (flags.qv_min_count != 1 && flags.qv_filename.empty() && flags.qv_bed_filename.empty() && !flags.kmer_guard && flags.kmer_fix_filename.empty() &&
        flags.kmer_bridge_filename.empty() && flags.qv_cn_filename.empty()) {   // (1 is the run without the flag)
        std::fprintf(stderr, "[Hypo::] Error: Arg Error: --qv-min-count changes what --qv, --qv-bed, --kmer-guard, --guard-records and --kmer-fix ask the reads: it needs at least one of them!\n");
        std::exit(1);
    }
    if (bridge_opts && flags.kmer_bridge_filename.empty()) {
        std::fprintf(stderr, "[Hypo::] Error: Arg Error: --kmer-bridge-max and --kmer-bridge-slack set how --kmer-bridge searches: they need --kmer-bridge!\n");
        std::exit(1);
    }
    if (flags.kmer_bridge_vote && flags.kmer_bridge_filename.empty()) {
        std::fprintf(stderr, "[Hypo::] Error: Arg Error: --kmer-bridge-vote (2 to 255) settles what --kmer-bridge leaves ambiguous: it needs --kmer-bridge!\n");
        std::exit(1);
    }
    if (!flags.qv_save_filename.empty() && !flags.qv_load_filename.empty()) {
        std::fprintf(stderr, "[Hypo::] Error: Arg Error: --qv-save stores the k-mer set a run builds from the reads, --qv-load takes it from a file instead: give one of them!\n");
        std::exit(1);
    }
    if (!flags.qv_load_filename.empty() && flags.qv_filename.empty() && flags.qv_bed_filename.empty() && flags.qv_spectra_filename.empty() && !flags.kmer_guard &&
        flags.kmer_fix_filename.empty() && flags.kmer_bridge_filename.empty() && flags.qv_cn_filename.empty()) {
        std::fprintf(stderr, "[Hypo::] Error: Arg Error: --qv-load fills the k-mer set that --qv, --qv-bed, --qv-spectra, --kmer-guard, --kmer-fix and --kmer-bridge ask: it needs at least one of them!\n");
        std::exit(1);
    }
    if (!(is_sr && is_draft && is_size && is_bamsr && is_cov)) {
        std::fprintf(stderr, "[Hypo::] Error: Invalid command: Too few arguments!\n");
        usage();
        return 1;
    }
    if (flags.output_filename.empty()) {                                  // src/main.cpp:317-323
        const size_t s = flags.draft_filename.find_last_of("(/\\");
        std::string full = flags.draft_filename.substr(s == std::string::npos ? 0 : s + 1);
        flags.output_filename = "hypo_" + full.substr(0, full.find_last_of(".")) + ".fasta";
    }
    mkdir(HYPO_AUX_DIR, 0777);
    flags.done_stage = 0;
    if (flags.intermed && file_exists(HYPO_STAGEFILE)) {                  // last stage number of aux/stage.txt (src/main.cpp:327-345)
        std::ifstream ifs(HYPO_STAGEFILE);
        std::string a, b, c; unsigned st = 0;
        while (ifs >> a >> b >> c >> st) {}
        flags.done_stage = st;
        std::cout << "Stagenum found is " << st << std::endl;
    }
    std::fprintf(stdout, "[Hypo::Utils] Info: Beginning from stage: %u\n", flags.done_stage);
    const bool timing = std::getenv("HYPO_HOST_TIMING") != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    auto since = [&]() { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); };
    if (flags.devices.empty()) {                                           // --device D, or --gpus N = devices 0..N-1
        if (flags.gpus > 1) for (int d = 0; d < flags.gpus; ++d) flags.devices.push_back(d);
        else flags.devices.push_back(flags.device);
    }
    // HYPO_GIANT_ARENA_MB: HBM per device context for the windows beyond the table-driven size classes (size class 6; default 1024, 0 = none:
    // such windows then keep their draft with a warning, as before round 6)
    if (const char* ga = std::getenv("HYPO_GIANT_ARENA_MB")) {
        if (hypo_gpu_set_option("giant_arena_mb", std::atoi(ga)) != HYPO_OK) { std::fprintf(stderr, "[Hypo::] Error: %s\n", hypo_gpu_last_error()); return 1; }
    }
    if (hypo_gpu_init(flags.devices.data(), (int)flags.devices.size()) != HYPO_OK) { std::fprintf(stderr, "[Hypo::] Error: %s\n", hypo_gpu_last_error()); return 1; }
    if (flags.native_klov && hypo_gpu_set_option("native_klov", 1) != HYPO_OK) { std::fprintf(stderr, "[Hypo::] Error: %s\n", hypo_gpu_last_error()); return 1; }
    if (flags.ccs_windows) { hypo::Window_settings.ideal_swind_size = 500; hypo::Window_settings.wind_size_search_th = 400; }   // src/main.cpp:577-580
    if (timing) std::fprintf(stderr, "[timing] main: device initialised at %.3f s\n", since());
    {
        hypo::Hypo h(flags);
        if (const char* d = std::getenv("HYPO_REGION_DUMP")) h.set_region_dump(d);
        h.polish();
        if (timing) std::fprintf(stderr, "[timing] main: polish() returned at %.3f s\n", since());
    }
    if (timing) std::fprintf(stderr, "[timing] main: pipeline objects released at %.3f s\n", since());
    return 0;
}
