// RunOutputs.hpp — the result files of one run: the polished FASTA, the VCF (--vcf), the QV table (--qv), its track (--qv-bed), the
// k-mer spectra (--qv-spectra), the list of k-mer fixes (--kmer-fix), the list of k-mer bridges (--kmer-bridge) and the copy-number
// bins (--qv-cn).
// The records go to <output>.tmp, which takes the output's name only when every contig is in it and the file closed without an error:
// a run that fails half way (a device error, a bad record three batches in) leaves no truncated file under the name the caller asked
// for, and an earlier result under that name stays what it was.  A failing run removes its .tmp on the way out.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <functional>
#include <string>

namespace hypo {

class RunOutputs {
public:
    enum Which { FASTA = 0, VCF = 1, QV = 2, BED = 3, SPECTRA = 4, FIXES = 5, BRIDGES = 6, CN = 7, N_FILES = 8 };
    RunOutputs() {
        static bool cleanup_registered = false;
        if (!cleanup_registered) { cleanup_registered = true; std::atexit(discard); }
        live() = this;
    }
    ~RunOutputs() { live() = nullptr; }
    // <name>.tmp is created; a file that cannot be opened ends the run
    std::ofstream& open_fasta(const std::string& name) { return open(FASTA, name); }
    std::ofstream& open_vcf(const std::string& name) { return open(VCF, name); }          // (the VCF follows the FASTA: <vcf>.tmp until the run succeeds)
    std::ofstream& open_qv(const std::string& name) { return open(QV, name); }
    std::ofstream& open_bed(const std::string& name) { return open(BED, name); }
    std::ofstream& open_spectra(const std::string& name) { return open(SPECTRA, name); }
    std::ofstream& open_fixes(const std::string& name) { return open(FIXES, name); }
    std::ofstream& open_bridges(const std::string& name) { return open(BRIDGES, name); }
    std::ofstream& open_cn(const std::string& name) { return open(CN, name); }
    std::ofstream& fasta() { return _f[FASTA].os; }
    std::ofstream& vcf() { return _f[VCF].os; }
    // every file is closed and checked before any takes its name, FASTA, VCF, QV, BED, spectra, fixes, bridges, copy number in this order (`renamed` after each); a file that
    // cannot take its name takes those before it with it
    void commit(const std::function<void(Which)>& renamed) {
        static const char* const label[N_FILES] = {"output", "VCF", "QV", "QV track", "QV spectra", "k-mer fix", "k-mer bridge", "copy number"};
        for (int i = 0; i < N_FILES; ++i) {
            if (_f[i].tmp.empty()) continue;
            _f[i].os.close();
            if (!_f[i].os) { std::fprintf(stderr, "[Hypo::Hypo] Error: writing the %s file (%s) failed!\n", label[i], _f[i].tmp.c_str()); std::exit(1); }
        }
        for (int i = 0; i < N_FILES; ++i) {
            if (_f[i].tmp.empty()) continue;
            if (std::rename(_f[i].tmp.c_str(), _f[i].name.c_str()) != 0) {
                std::fprintf(stderr, "[Hypo::Hypo] Error: could not move %s to %s!\n", _f[i].tmp.c_str(), _f[i].name.c_str());
                for (int j = 0; j < i; ++j) if (!_f[j].name.empty()) std::remove(_f[j].name.c_str());
                std::exit(1);
            }
            _f[i].tmp.clear();
            renamed((Which)i);
        }
    }
    // what a failing run leaves behind goes: the exit handler, and the helper threads before they leave with _Exit
    static void discard() {
        if (!live()) return;
        for (const File& f : live()->_f) if (!f.tmp.empty()) std::remove(f.tmp.c_str());
    }

private:
    struct File { std::string name, tmp; std::ofstream os; };      // tmp: <name>.tmp while the run is writing it
    File _f[N_FILES];
    static RunOutputs*& live() { static RunOutputs* p = nullptr; return p; }
    std::ofstream& open(Which w, const std::string& name) {
        static const char* const label[N_FILES] = {"Output", "VCF", "QV", "QV track", "QV spectra", "k-mer fix", "k-mer bridge", "copy number"};
        File& f = _f[w];
        f.name = name; f.tmp = name + ".tmp";
        f.os.open(f.tmp);
        if (!f.os.is_open()) { std::fprintf(stderr, "[Hypo::Hypo] Error: File open error: %s File (%s) could not be opened!\n", label[w], f.tmp.c_str()); std::exit(1); }
        return f.os;
    }
};

}  // namespace hypo
