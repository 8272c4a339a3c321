"""ctypes binding of libhypo_gpu.so (the C-ABI of include/hypo_gpu.h) + torch device-memory plumbing.

There is no Python or CPU implementation of the hot path behind this module: if the HIP library is
missing or no gfx950 device is present, loading / init raises.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from . import abi
from .batch import HostBatch

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "_build", "libhypo_gpu.so")

EXPORTS = [
    "hypo_gpu_init", "hypo_gpu_shutdown", "hypo_gpu_abi_version", "hypo_gpu_last_error",
    "hypo_gpu_num_cus", "hypo_gpu_solid_scan", "hypo_gpu_solid_scan_workspace_bytes",
    "hypo_gpu_solid_scan_device", "hypo_gpu_poa_batch", "hypo_gpu_poa_workspace_bytes",
    "hypo_gpu_poa_batch_device", "hypo_gpu_poa_slot_layout", "hypo_gpu_poa_last_stats",
    "hypo_gpu_poa_read_stats", "hypo_gpu_profile_begin", "hypo_gpu_profile_calls", "hypo_gpu_profile_read",
    "hypo_gpu_num_devices", "hypo_gpu_use_device", "hypo_gpu_build_id", "hypo_gpu_solid_set_upload",
    "hypo_gpu_poa_batch_sharded", "hypo_gpu_poa_batch_begin", "hypo_gpu_poa_batch_end", "hypo_gpu_set_option",
    "hypo_gpu_arms_build", "hypo_gpu_arms_download", "hypo_gpu_arms_poa",
    "hypo_gpu_arms_build_long", "hypo_gpu_arms_download_long", "hypo_gpu_arms_poa_long",
    "hypo_gpu_reads_upload", "hypo_gpu_support_kmers", "hypo_gpu_support_minimizers",
    "hypo_gpu_solid_scan_keep", "hypo_gpu_solid_release", "hypo_gpu_support_kmers_kept", "hypo_gpu_host_alloc", "hypo_gpu_host_free", "hypo_gpu_host_register", "hypo_gpu_host_unregister",
    "hypo_gpu_kmer_count_begin", "hypo_gpu_kmer_count_add", "hypo_gpu_kmer_histogram", "hypo_gpu_solid_set_build",
    "hypo_gpu_kmer_count_end", "hypo_gpu_edit_scripts", "hypo_gpu_edit_last_counts",
    "hypo_gpu_kset_begin", "hypo_gpu_kset_add", "hypo_gpu_kset_size", "hypo_gpu_kset_query", "hypo_gpu_kset_end",
    "hypo_gpu_kset_query_spans", "hypo_gpu_kset_query_variants", "hypo_gpu_kset_query_track", "hypo_gpu_kset_query_fixes",
    "hypo_gpu_kset_query_walks", "hypo_gpu_kset_query_walk_sets",
    "hypo_gpu_kset_counts_enable", "hypo_gpu_kset_mark", "hypo_gpu_kset_spectrum", "hypo_gpu_kset_min_count",
    "hypo_gpu_kset_export", "hypo_gpu_kset_import", "hypo_gpu_kset_query_depth",
]
KSET_SPAN_PIECE = 2048        # windows per piece of a long span (kset_kernel.hpp)
KSET_MAX_EDITS = 12           # edits of a site of hypo_gpu_kset_query_variants (HYPO_KSET_MAX_EDITS)


class HypoGpuError(RuntimeError):
    pass


def build_library() -> str:
    """Compiles hypo_amd/csrc for gfx950 with hipcc (works without a GPU)."""
    subprocess.check_call(["make", "-s", "-j4", "-C", os.path.join(HERE, "csrc")])
    return LIB_PATH


def load_library(path: str = LIB_PATH) -> C.CDLL:
    if not os.path.exists(path):
        raise HypoGpuError(f"{path} is missing: build it with `make -C hypo_amd/csrc` "
                           "(python -c 'import __graft_entry__ as g; g.build()'); there is no CPU fallback")
    # One HIP runtime per process: torch bundles its own libamdhip64.so.7; importing it first makes the
    # loader resolve this library's NEEDED libamdhip64.so.7 to the same copy (two runtimes in one
    # process cannot both own the GPU).
    import torch  # noqa: F401
    lib = C.CDLL(path)
    lib.hypo_gpu_last_error.restype = C.c_char_p
    lib.hypo_gpu_build_id.restype = C.c_char_p
    lib.hypo_gpu_poa_workspace_bytes.restype = C.c_size_t
    lib.hypo_gpu_solid_scan_workspace_bytes.restype = C.c_size_t
    lib.hypo_gpu_solid_scan_workspace_bytes.argtypes = [C.c_uint64]
    lib.hypo_gpu_poa_workspace_bytes.argtypes = [C.c_uint32, C.c_uint32]
    for name in EXPORTS:
        getattr(lib, name)
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def host_struct(b: HostBatch) -> abi.WindowBatch:
    s = abi.WindowBatch()
    s.n_windows, s.n_arms = b.n_windows, b.n_arms
    s.windows, s.draft4, s.draft4_bytes = _p(b.windows), _p(b.draft4), b.draft4.size
    s.arm_off, s.arm_len, s.arms2, s.arms2_bytes = _p(b.arm_off), _p(b.arm_len), _p(b.arms2), b.arms2.size
    return s


class HypoGpu:
    """One process = one GPU (rank-local), mirroring the reference's single Hypo object."""

    def __init__(self, device: int = 0, path: str = LIB_PATH, devices=None):
        """devices: list of HIP device ids for several contexts in this process (hypo_gpu_poa_batch_sharded); the torch
        plumbing of the *_device entry points uses context 0 = `device`."""
        self.lib = load_library(path)
        if self.lib.hypo_gpu_abi_version() != abi.ABI_VERSION:
            raise HypoGpuError("ABI version mismatch between hypo_amd/abi.py and libhypo_gpu.so")
        devices = [device] if devices is None else list(devices)
        self.device = devices[0]
        ids = (C.c_int * len(devices))(*devices)
        self._check(self.lib.hypo_gpu_init(ids, C.c_int(len(devices))))
        self.num_cus = int(self.lib.hypo_gpu_num_cus())

    def _check(self, rc):
        if rc != 0:
            raise HypoGpuError(f"libhypo_gpu rc={rc}: {self.lib.hypo_gpu_last_error().decode()}")

    # ---- host-buffer entry points (H2D + kernels + D2H inside the library) -----------------------------
    def poa_batch(self, b: HostBatch, scores=abi.DEFAULT_SCORES, off=None):
        """Returns (bases u8, off u64, len u32, status u8)."""
        sp = abi.ScoreParams(*scores)
        n = b.n_windows
        if off is None:
            off = np.zeros(n + 1, dtype=np.uint64)
            ins = host_struct(b)
            self._check(self.lib.hypo_gpu_poa_slot_layout(C.byref(ins), _p(off)))
        bases = np.zeros(int(off[-1]) + 1, dtype=np.uint8)
        ln = np.zeros(n, dtype=np.uint32)
        st = np.zeros(n, dtype=np.uint8)
        ins = host_struct(b)
        out = abi.ConsensusBatch(_p(bases), _p(off), _p(ln), _p(st))
        self._check(self.lib.hypo_gpu_poa_batch(C.byref(sp), C.byref(ins), C.byref(out)))
        return bases, off, ln, st

    def poa_batch_sharded(self, b: HostBatch, scores=abi.DEFAULT_SCORES, off=None):
        """hypo_gpu_poa_batch over all contexts of this process.  Returns (bases u8, off u64, len u32, status u8)."""
        sp = abi.ScoreParams(*scores)
        n = b.n_windows
        if off is None:
            off = b.slot_layout()
        bases = np.zeros(int(off[-1]) + 1, dtype=np.uint8)
        ln = np.zeros(n, dtype=np.uint32)
        st = np.zeros(n, dtype=np.uint8)
        ins = host_struct(b)
        out = abi.ConsensusBatch(_p(bases), _p(off), _p(ln), _p(st))
        self._check(self.lib.hypo_gpu_poa_batch_sharded(C.byref(sp), C.byref(ins), C.byref(out)))
        return bases, off, ln, st

    def poa_batch_begin(self, b: HostBatch, off, bases, ln, st, scores=abi.DEFAULT_SCORES, no_arm_off=False):
        """hypo_gpu_poa_batch_begin on caller-owned buffers; returns (ticket, keep-alive objects).  no_arm_off: the arms of `b`
        lie back to back (HostBatch built by this package), let the device compute their offsets."""
        sp = abi.ScoreParams(*scores)
        ins = host_struct(b)
        if no_arm_off:
            ins.arm_off = None
        out = abi.ConsensusBatch(_p(bases), _p(off), _p(ln), _p(st))
        t = C.c_int(-1)
        self._check(self.lib.hypo_gpu_poa_batch_begin(C.byref(sp), C.byref(ins), C.byref(out), C.byref(t)))
        return int(t.value), (sp, ins, out)

    def poa_batch_end(self, ticket: int):
        self._check(self.lib.hypo_gpu_poa_batch_end(C.c_int(ticket)))

    def poa_consensus(self, b: HostBatch, scores=abi.DEFAULT_SCORES, off=None):
        bases, off, ln, st = self.poa_batch(b, scores, off)
        cons = [bases[int(off[i]):int(off[i]) + int(ln[i])].tobytes().decode() if st[i] == 0 else None
                for i in range(b.n_windows)]
        return cons, st

    def last_stats(self) -> dict:
        s = abi.PoaStats()
        self._check(self.lib.hypo_gpu_poa_last_stats(C.byref(s)))
        return _stats_dict(s)

    # ---- the solid k-mer set from the short reads (ABI 9) ---------------------------------------------------------------
    def kmer_count_begin(self, k: int, coverage: int):
        self._check(self.lib.hypo_gpu_kmer_count_begin(C.c_uint32(k), C.c_uint32(coverage)))
        self._kmer_k = k

    def kmer_count_add(self, data):
        """data: bytes / bytearray / uint8 array of sequence bytes; any byte other than ACGTacgt ends a run of bases"""
        a = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)
        self._check(self.lib.hypo_gpu_kmer_count_add(_p(a), C.c_uint64(a.size)))

    def kmer_histogram(self, coverage: int) -> np.ndarray:
        hist = np.zeros(4 * coverage + 1, dtype=np.uint64)
        self._check(self.lib.hypo_gpu_kmer_histogram(_p(hist), C.c_uint32(hist.size)))
        return hist

    def solid_set_build(self, lower: int, upper: int, exclude_hp=True):
        """(bits u64[4^k / 64], set bits, canonical solid k-mers) of the table of the last kmer_count_begin"""
        bits = np.zeros((1 << (2 * self._kmer_k)) // 64, dtype=np.uint64)
        nb, nc = C.c_uint64(0), C.c_uint64(0)
        self._check(self.lib.hypo_gpu_solid_set_build(C.c_uint32(lower), C.c_uint32(upper), C.c_int(1 if exclude_hp else 0),
                                                      _p(bits), C.byref(nb), C.byref(nc)))
        return bits, int(nb.value), int(nc.value)

    def kmer_count_end(self):
        self._check(self.lib.hypo_gpu_kmer_count_end())

    def solid_kmers_build(self, paths_or_bytes, k: int, coverage: int, chunk=None):
        """The solid k-mer set of a run without -i.  paths_or_bytes: a list of read files (FASTA / FASTQ, plain or gzip; parsed by
        the host library's streaming parser, SolidBuild.cpp) or sequence bytes (bytes, or a list of byte strings counted one
        hypo_gpu_kmer_count_add call each; `chunk` cuts one byte string into calls of that many bytes, k - 1 bytes overlapping).
        Returns a dict: hist, cut = (err, mean, lower, upper) or None when the reference's result is undefined, bits, n_bits,
        n_canonical (and for files: seq_bytes, file_bytes, times = (parse, count, histogram, set, total) in seconds)."""
        if isinstance(paths_or_bytes, (str, os.PathLike)) or (isinstance(paths_or_bytes, (list, tuple)) and paths_or_bytes
                                                             and isinstance(paths_or_bytes[0], (str, os.PathLike))):
            paths = [paths_or_bytes] if isinstance(paths_or_bytes, (str, os.PathLike)) else list(paths_or_bytes)
            return self._solid_build_files([os.fspath(p) for p in paths], k, coverage)
        from .host import LIB_PATH as HOST_LIB
        host = C.CDLL(HOST_LIB)
        pieces = [paths_or_bytes] if isinstance(paths_or_bytes, (bytes, bytearray)) else list(paths_or_bytes)
        self.kmer_count_begin(k, coverage)
        try:
            for piece in pieces:
                if chunk:
                    at = 0
                    while True:
                        self.kmer_count_add(piece[at:at + chunk])
                        if at + chunk >= len(piece):
                            break
                        at += chunk - (k - 1)
                else:
                    self.kmer_count_add(piece)
            hist = self.kmer_histogram(coverage)
            cut = (C.c_uint32 * 4)()
            if host.hypo_host_solid_cutoffs(_p(hist), C.c_uint32(hist.size), cut) != 0:
                return {"hist": hist, "cut": None}
            cut = tuple(int(x) for x in cut)
            bits, nb, nc = self.solid_set_build(cut[2], cut[3])
            return {"hist": hist, "cut": cut, "bits": bits, "n_bits": nb, "n_canonical": nc}
        finally:
            self.kmer_count_end()

    # ---- edit scripts of replacement units (ABI 10; hypo --vcf) -------------------------------------------------------------
    def edit_scripts_raw(self, a_list, b_list, runs_cap=None):
        """(dist u32[n], run_off u64[n + 1], runs u32[]) of hypo_gpu_edit_scripts; runs = (len << 2) | op, op 0..3 = '=XDI'.
        A first runs_cap that is too small is answered with HYPO_E_WORKSPACE and the call is repeated with the size it reported (the
        library kept its results: the repeat only copies them out)."""
        def as_bytes(x):
            return x.encode() if isinstance(x, str) else bytes(x)
        a_list, b_list = [as_bytes(x) for x in a_list], [as_bytes(x) for x in b_list]
        if len(a_list) != len(b_list):
            raise ValueError("a_list and b_list differ in length")
        n = len(a_list)
        a_off = np.zeros(n + 1, dtype=np.uint64)
        b_off = np.zeros(n + 1, dtype=np.uint64)
        a_off[1:] = np.cumsum([len(x) for x in a_list], dtype=np.uint64)
        b_off[1:] = np.cumsum([len(x) for x in b_list], dtype=np.uint64)
        a = np.frombuffer(b"".join(a_list) + b"\0", dtype=np.uint8)
        b = np.frombuffer(b"".join(b_list) + b"\0", dtype=np.uint8)
        batch = abi.EditBatch()
        batch.n_pairs, batch.a, batch.a_off, batch.b, batch.b_off = n, _p(a), _p(a_off), _p(b), _p(b_off)
        dist = np.zeros(max(n, 1), dtype=np.uint32)
        run_off = np.zeros(n + 1, dtype=np.uint64)
        cap = 4 * n + 16 if runs_cap is None else runs_cap
        runs = np.zeros(max(cap, 1), dtype=np.uint32)
        rc = self.lib.hypo_gpu_edit_scripts(C.byref(batch), _p(dist), _p(run_off), _p(runs), C.c_uint64(cap))
        if rc == abi.HYPO_E_WORKSPACE:
            cap = int(run_off[n])
            runs = np.zeros(max(cap, 1), dtype=np.uint32)
            rc = self.lib.hypo_gpu_edit_scripts(C.byref(batch), _p(dist), _p(run_off), _p(runs), C.c_uint64(cap))
        self._check(rc)
        return dist[:n], run_off, runs[:int(run_off[n])]

    def edit_scripts(self, a_list, b_list):
        """a_list, b_list: bytes (or str).  (dist: u32 array, cigars: list of str) — the canonical unit-cost alignment of every a (draft span) against its b, as
        extended CIGARs in draft order ('=' match, 'X' substitution, 'D' draft base removed, 'I' base inserted)."""
        dist, run_off, runs = self.edit_scripts_raw(a_list, b_list)
        ops = "=XDI"
        cigars = ["".join(f"{int(r) >> 2}{ops[int(r) & 3]}" for r in runs[int(run_off[i]):int(run_off[i + 1])]) for i in range(len(dist))]
        return dist, cigars

    EDIT_COUNTS = ("pairs", "long", "wide", "second", "runs", "passes", "long_launches", "wide_launches")

    def edit_last_counts(self):
        """hypo_gpu_edit_last_counts as a dict: what the last computing edit_scripts call on this thread's context did"""
        out = np.zeros(8, dtype=np.uint64)
        self._check(self.lib.hypo_gpu_edit_last_counts(_p(out)))
        return dict(zip(self.EDIT_COUNTS, (int(x) for x in out)))

    def set_option(self, name: str, value: int):
        self._check(self.lib.hypo_gpu_set_option(name.encode(), C.c_int(value)))

    # ---- the exact k-mer set of the reads (ABI 11; hypo --qv) ---------------------------------------------------------------
    def use_device(self, slot: int):
        self._check(self.lib.hypo_gpu_use_device(C.c_int(slot)))

    def kset_begin(self, k: int, expected_distinct: int = 0, max_bytes: int = 0):
        self._check(self.lib.hypo_gpu_kset_begin(C.c_uint32(k), C.c_uint64(expected_distinct), C.c_uint64(max_bytes)))

    def kset_add_rc(self, data) -> int:
        """the return code of hypo_gpu_kset_add (HYPO_E_CAPACITY is an answer, not a failure of the binding)"""
        a = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)
        return int(self.lib.hypo_gpu_kset_add(_p(a), C.c_uint64(a.size)))

    def kset_add(self, data):
        self._check(self.kset_add_rc(data))

    def kset_size(self):
        """(distinct k-mers in the set, bytes of its table)"""
        n, b = C.c_uint64(0), C.c_uint64(0)
        self._check(self.lib.hypo_gpu_kset_size(C.byref(n), C.byref(b)))
        return int(n.value), int(b.value)

    def kset_query(self, seqs):
        """seqs: byte strings.  (total u64[n], missing u64[n]): the ACGT-only windows of every sequence and those not in the set"""
        seqs = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
        n = len(seqs)
        off = np.zeros(n + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
        data = np.frombuffer(b"".join(seqs) + b"\0", dtype=np.uint8)
        total = np.zeros(max(n, 1), dtype=np.uint64)
        missing = np.zeros(max(n, 1), dtype=np.uint64)
        self._check(self.lib.hypo_gpu_kset_query(_p(data), _p(off), C.c_uint32(n), _p(total), _p(missing)))
        return total[:n], missing[:n]

    def kset_query_spans_rc(self, data, lo, hi):
        """(return code, total u64[n], missing u64[n]) of hypo_gpu_kset_query_spans; nothing is checked here"""
        a = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)
        lo = np.ascontiguousarray(lo, dtype=np.uint64)
        hi = np.ascontiguousarray(hi, dtype=np.uint64)
        assert lo.shape == hi.shape and lo.ndim == 1
        n = lo.size
        total = np.zeros(max(n, 1), dtype=np.uint64)
        missing = np.zeros(max(n, 1), dtype=np.uint64)
        pad = np.concatenate([a, np.zeros(1, np.uint8)])                # (an empty text still has an address)
        rc = int(self.lib.hypo_gpu_kset_query_spans(_p(pad), C.c_uint64(a.size), _p(lo), _p(hi), C.c_uint32(n), _p(total), _p(missing)))
        return rc, total[:n], missing[:n]

    def kset_query_spans(self, data, lo, hi):
        """span s = data[lo[s]:hi[s]].  (total u64[n], missing u64[n]) as kset_query gives them for the spans as sequences"""
        rc, total, missing = self.kset_query_spans_rc(data, lo, hi)
        self._check(rc)
        return total, missing

    def kset_query_variants_rc(self, data, alts, lo, hi, edit_off, eb, ee, ao, al, variants=True):
        """(return code, best_mask u32[n], best_total u64[n], best_missing u64[n], var_total, var_missing) of
        hypo_gpu_kset_query_variants; nothing is checked here.  var_*: u64[sum of 2^edits] as far as edit_off is sane, None
        without `variants`."""
        a = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)
        b = np.frombuffer(bytes(alts), dtype=np.uint8) if not isinstance(alts, np.ndarray) else np.ascontiguousarray(alts, dtype=np.uint8)
        lo, hi = np.ascontiguousarray(lo, dtype=np.uint64), np.ascontiguousarray(hi, dtype=np.uint64)
        edit_off = np.ascontiguousarray(edit_off, dtype=np.uint32)
        eb, ee, ao = (np.ascontiguousarray(x, dtype=np.uint64) for x in (eb, ee, ao))
        al = np.ascontiguousarray(al, dtype=np.uint32)
        n = lo.size
        assert hi.size == n and edit_off.size == n + 1
        pad = lambda x, t: np.concatenate([x, np.zeros(1, t)])          # (an empty array still has an address)
        n_edits = np.diff(edit_off.astype(np.int64))
        n_vars = int(sum(1 << int(e) for e in n_edits if 0 <= e <= 16))
        best_mask, best_total, best_missing = np.zeros(n + 1, np.uint32), np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)
        var_total = np.zeros(n_vars + 1, np.uint64) if variants else None
        var_missing = np.zeros(n_vars + 1, np.uint64) if variants else None
        rc = int(self.lib.hypo_gpu_kset_query_variants(
            _p(pad(a, np.uint8)), C.c_uint64(a.size), _p(pad(b, np.uint8)), C.c_uint64(b.size), _p(pad(lo, np.uint64)), _p(pad(hi, np.uint64)), _p(edit_off),
            C.c_uint32(n), _p(pad(eb, np.uint64)), _p(pad(ee, np.uint64)), _p(pad(ao, np.uint64)), _p(pad(al, np.uint32)), _p(best_mask), _p(best_total),
            _p(best_missing), _p(var_total) if variants else None, _p(var_missing) if variants else None))
        return rc, best_mask[:n], best_total[:n], best_missing[:n], (var_total[:n_vars] if variants else None), (var_missing[:n_vars] if variants else None)

    def kset_query_variants(self, data, alts, lo, hi, edit_off, eb, ee, ao, al, variants=True):
        """site s = data[lo[s]:hi[s]] with the edits edit_off[s] .. edit_off[s + 1] (edit e: data[eb[e]:ee[e]] -> alts[ao[e]:ao[e] + al[e]]).
        (best_mask, best_total, best_missing, var_total, var_missing): per site the best subset of its edits (fewest missing, most
        edits, greatest mask), and every subset's pair in site and mask order."""
        out = self.kset_query_variants_rc(data, alts, lo, hi, edit_off, eb, ee, ao, al, variants)
        self._check(out[0])
        return out[1:]

    def kset_query_track_rc(self, seqs_or_text, off=None, want=None, iv_cap=0):
        """(return code, total u64[n], missing u64[n], iv_off u64[n + 1], iv_start, iv_end, iv_missing: u64[iv_cap]) of one call of
        hypo_gpu_kset_query_track; nothing is checked here.  A list of byte strings, or one text with its n + 1 offsets.  The three
        interval arrays are filled with abi.TRACK_UNTOUCHED before the call (iv_cap = 0: the counting call, NULL pointers)."""
        if off is None:
            seqs = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs_or_text]
            off = np.zeros(len(seqs) + 1, dtype=np.uint64)
            off[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
            text = b"".join(seqs)
        else:
            text = seqs_or_text.encode() if isinstance(seqs_or_text, str) else bytes(seqs_or_text)
            off = np.ascontiguousarray(off, dtype=np.uint64)
        n = off.size - 1
        data = np.frombuffer(text + b"\0", dtype=np.uint8)               # (an empty text still has an address)
        if want is not None:
            want = np.ascontiguousarray(want, dtype=np.uint8)
            assert want.size == n
        total, missing = np.zeros(max(n, 1), dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint64)
        iv_off = np.zeros(n + 1, dtype=np.uint64)
        iv = [np.full(iv_cap, abi.TRACK_UNTOUCHED, dtype=np.uint64) for _ in range(3)]
        rc = int(self.lib.hypo_gpu_kset_query_track(_p(data), _p(off), C.c_uint32(n), _p(want) if want is not None and n else None, _p(total), _p(missing),
                                                    _p(iv_off), *[_p(a) if iv_cap else None for a in iv], C.c_uint64(iv_cap)))
        return (rc, total[:n], missing[:n], iv_off) + tuple(iv)

    def kset_query_track(self, seqs_or_text, off=None, want=None):
        """kset_query, and where the missing windows are: (total u64[n], missing u64[n], iv_off u64[n + 1], iv_start, iv_end,
        iv_missing).  The intervals of sequence s are [iv_off[s], iv_off[s + 1]) of the three arrays: maximal runs [start, end) of
        bases under a missing window, relative to the sequence, ascending, with the missing windows inside.  want[s] == 0: no
        intervals for s.  Two calls: one that counts, one with room."""
        out = self.kset_query_track_rc(seqs_or_text, off, want, 0)
        if out[0] == abi.HYPO_E_WORKSPACE:
            out = self.kset_query_track_rc(seqs_or_text, off, want, int(out[3][-1]))
        self._check(out[0])
        return out[1:]

    def kset_query_fixes_rc(self, data, lo, hi, c0, c1, cands=True):
        """(return code, none_total u64[n], none_missing u64[n], best_cand u32[n], best_total u64[n], best_missing u64[n], zeros u32[n],
        cand_total, cand_missing) of hypo_gpu_kset_query_fixes; nothing is checked here.  cand_*: u64[sum of 9 (c1 - c0) - 3] as far as
        the regions are sane, None without `cands`.  Every output is filled with abi.FIXES_UNTOUCHED64 / 32 before the call."""
        a = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)
        lo, hi, c0, c1 = (np.ascontiguousarray(x, dtype=np.uint64) for x in (lo, hi, c0, c1))
        n = lo.size
        assert hi.size == n and c0.size == n and c1.size == n
        pad = lambda x, t: np.concatenate([x, np.zeros(1, t)])          # (an empty array still has an address)
        w = c1.astype(np.int64) - c0.astype(np.int64)
        n_cands = int(sum(9 * int(x) - 3 for x in w if 1 <= x <= abi.KSET_MAX_FIX_REGION))
        u64 = lambda m: np.full(m + 1, abi.FIXES_UNTOUCHED64, np.uint64)
        u32 = lambda m: np.full(m + 1, abi.FIXES_UNTOUCHED32, np.uint32)
        nt, nm, bc, bt, bm, z = u64(n), u64(n), u32(n), u64(n), u64(n), u32(n)
        ct, cm = (u64(n_cands), u64(n_cands)) if cands else (None, None)
        rc = int(self.lib.hypo_gpu_kset_query_fixes(
            _p(pad(a, np.uint8)), C.c_uint64(a.size), _p(pad(lo, np.uint64)), _p(pad(hi, np.uint64)), _p(pad(c0, np.uint64)), _p(pad(c1, np.uint64)), C.c_uint32(n),
            _p(nt), _p(nm), _p(bc), _p(bt), _p(bm), _p(z), _p(ct) if cands else None, _p(cm) if cands else None))
        return rc, nt[:n], nm[:n], bc[:n], bt[:n], bm[:n], z[:n], (ct[:n_cands] if cands else None), (cm[:n_cands] if cands else None)

    def kset_query_fixes(self, data, lo, hi, c0, c1, cands=True):
        """site s = data[lo[s]:hi[s]] with the region [c0[s], c1[s]) of w bytes; its 9 w - 3 candidates are the span as it is, then
        every substitution, deletion and insertion of one base in the region (include/hypo_gpu.h has the order).  (none_total,
        none_missing, best_cand, best_total, best_missing, zeros, cand_total, cand_missing): the unedited span's pair, the canonical
        candidate with the fewest missing windows, how many canonical candidates miss nothing, and every candidate's pair."""
        out = self.kset_query_fixes_rc(data, lo, hi, c0, c1, cands)
        self._check(out[0])
        return out[1:]

    def kset_query_walks_rc(self, data, frm, to, dlo, dhi, budget):
        """(return code, status u32[n], steps u32[n], len u32[n], walk u8[n, abi.KSET_MAX_WALK]) of hypo_gpu_kset_query_walks; nothing
        is checked here.  Every output is filled with abi.WALKS_UNTOUCHED32 / 8 before the call."""
        a = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)
        frm, to = (np.ascontiguousarray(x, dtype=np.uint64) for x in (frm, to))
        dlo, dhi = (np.ascontiguousarray(x, dtype=np.uint32) for x in (dlo, dhi))
        n = frm.size
        assert to.size == n and dlo.size == n and dhi.size == n
        pad = lambda x, t: np.concatenate([x, np.zeros(1, t)])          # (an empty array still has an address)
        u32 = lambda: np.full(n + 1, abi.WALKS_UNTOUCHED32, np.uint32)
        status, steps, ln = u32(), u32(), u32()
        walk = np.full((n + 1, abi.KSET_MAX_WALK), abi.WALKS_UNTOUCHED8, np.uint8)
        rc = int(self.lib.hypo_gpu_kset_query_walks(
            _p(pad(a, np.uint8)), C.c_uint64(a.size), _p(pad(frm, np.uint64)), _p(pad(to, np.uint64)), _p(pad(dlo, np.uint32)), _p(pad(dhi, np.uint32)), C.c_uint32(n),
            C.c_uint32(budget), _p(status), _p(steps), _p(ln), _p(walk)))
        return rc, status[:n], steps[:n], ln[:n], walk[:n]

    def kset_query_walks(self, data, frm, to, dlo, dhi, budget):
        """site s: the walks through the set from the k-mer data[frm[s]:frm[s] + k] that arrive at data[to[s]:to[s] + k] after dlo[s] ..
        dhi[s] steps, by the depth-first search of include/hypo_gpu.h with at most `budget` visits.  (status, steps, len, walk): one of
        abi.WALK_*, the visits made, and the first walk's length and bases (walk[s, :len[s]])."""
        out = self.kset_query_walks_rc(data, frm, to, dlo, dhi, budget)
        self._check(out[0])
        return out[1:]

    def kset_query_walk_sets_rc(self, data, frm, to, dlo, dhi, budget):
        """(return code, status u32[n], steps u32[n], n_walks u32[n], len u32[n, W], low u32[n, W], walk u8[n, W, abi.KSET_MAX_WALK]) of
        hypo_gpu_kset_query_walk_sets, W = abi.KSET_MAX_WALKS; nothing is checked here.  Every output is filled with
        abi.WALKS_UNTOUCHED32 / 8 before the call."""
        a = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)
        frm, to = (np.ascontiguousarray(x, dtype=np.uint64) for x in (frm, to))
        dlo, dhi = (np.ascontiguousarray(x, dtype=np.uint32) for x in (dlo, dhi))
        n = frm.size
        assert to.size == n and dlo.size == n and dhi.size == n
        pad = lambda x, t: np.concatenate([x, np.zeros(1, t)])          # (an empty array still has an address)
        u32 = lambda *shape: np.full((n + 1,) + shape, abi.WALKS_UNTOUCHED32, np.uint32)
        status, steps, nw, ln, low = u32(), u32(), u32(), u32(abi.KSET_MAX_WALKS), u32(abi.KSET_MAX_WALKS)
        walk = np.full((n + 1, abi.KSET_MAX_WALKS, abi.KSET_MAX_WALK), abi.WALKS_UNTOUCHED8, np.uint8)
        rc = int(self.lib.hypo_gpu_kset_query_walk_sets(
            _p(pad(a, np.uint8)), C.c_uint64(a.size), _p(pad(frm, np.uint64)), _p(pad(to, np.uint64)), _p(pad(dlo, np.uint32)), _p(pad(dhi, np.uint32)), C.c_uint32(n),
            C.c_uint32(budget), _p(status), _p(steps), _p(nw), _p(ln), _p(low), _p(walk)))
        return rc, status[:n], steps[:n], nw[:n], ln[:n], low[:n], walk[:n]

    def kset_query_walk_sets(self, data, frm, to, dlo, dhi, budget):
        """site s: up to abi.KSET_MAX_WALKS walks through the set from the k-mer data[frm[s]:frm[s] + k] that arrive at data[to[s]:to[s] + k]
        after dlo[s] .. dhi[s] steps, by the depth-first search of include/hypo_gpu.h with at most `budget` visits, on a set that counts.
        (status, steps, n_walks, len, low, walk): one of abi.WALK_*, the visits made, the walks reported and, for walk w < n_walks[s], its
        length, the least read count along it and its bases (walk[s, w, :len[s, w]])."""
        out = self.kset_query_walk_sets_rc(data, frm, to, dlo, dhi, budget)
        self._check(out[0])
        return out[1:]

    def kset_counts_enable_rc(self, n_texts: int) -> int:
        return int(self.lib.hypo_gpu_kset_counts_enable(C.c_uint32(n_texts)))

    def kset_counts_enable(self, n_texts: int):
        """after kset_begin, while the set is empty: kset_add counts every window from here on, and n_texts texts can be marked"""
        self._check(self.kset_counts_enable_rc(n_texts))

    def kset_mark_rc(self, text: int, seqs):
        """(return code, windows, unmarked windows) of one call of hypo_gpu_kset_mark; nothing is checked here"""
        seqs = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
        off = np.zeros(len(seqs) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
        data = np.frombuffer(b"".join(seqs) + b"\0", dtype=np.uint8)      # (an empty text still has an address)
        n_win, n_un = C.c_uint64(0), C.c_uint64(0)
        rc = int(self.lib.hypo_gpu_kset_mark(C.c_uint32(text), _p(data), _p(off), C.c_uint32(len(seqs)), C.byref(n_win), C.byref(n_un)))
        return rc, int(n_win.value), int(n_un.value)

    def kset_mark(self, text: int, seqs):
        """every window of the sequences adds 1 to its k-mer's copy number in `text`.  (windows, those whose k-mer is not in the set)"""
        rc, n_win, n_un = self.kset_mark_rc(text, seqs)
        self._check(rc)
        return n_win, n_un

    def kset_spectrum_rc(self, text: int):
        hist = np.zeros(abi.KSET_SPECTRUM_BINS, dtype=np.uint64)
        return int(self.lib.hypo_gpu_kset_spectrum(C.c_uint32(text), _p(hist))), hist.reshape(abi.KSET_SPECTRUM_ROWS, abi.KSET_SPECTRUM_COLS)

    def kset_spectrum(self, text: int) -> np.ndarray:
        """u64[256, 5]: [c, j] = the k-mers of the set seen c times in the reads (255: or more) and min(j, 4) times in `text`"""
        rc, hist = self.kset_spectrum_rc(text)
        self._check(rc)
        return hist

    def kset_min_count_rc(self, t: int) -> int:
        return int(self.lib.hypo_gpu_kset_min_count(C.c_uint32(t)))

    def kset_min_count(self, t: int):
        """on a set that counts: from the next call on the four queries answer against the k-mers the reads have at least t times
        (1..255; 1 = the set itself)"""
        self._check(self.kset_min_count_rc(t))

    def kset_query_depth_rc(self, seqs_or_text, off=None, bin=1024, text=0, unit=1, n_bins=None):
        """(return code, windows, missing, rated, over, under: u32[n_bins], med_count u8[n_bins]) of one call of
        hypo_gpu_kset_query_depth; nothing is checked here.  A list of byte strings, or one text with its n + 1 offsets.  n_bins None:
        the sum of ceil(length / bin).  The arrays are filled with abi.DEPTH_UNTOUCHED32 / 8 before the call."""
        if off is None:
            seqs = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs_or_text]
            off = np.zeros(len(seqs) + 1, dtype=np.uint64)
            off[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
            data = b"".join(seqs)
        else:
            data = seqs_or_text.encode() if isinstance(seqs_or_text, str) else bytes(seqs_or_text)
            off = np.ascontiguousarray(off, dtype=np.uint64)
        n = off.size - 1
        if n_bins is None:
            n_bins = int(sum(-(-int(l) // bin) for l in np.diff(off.astype(np.int64)))) if bin > 0 else 0
        buf = np.frombuffer(data + b"\0", dtype=np.uint8)                # (an empty text still has an address)
        u32 = [np.full(max(n_bins, 1), abi.DEPTH_UNTOUCHED32, dtype=np.uint32) for _ in range(5)]
        med = np.full(max(n_bins, 1), abi.DEPTH_UNTOUCHED8, dtype=np.uint8)
        rc = int(self.lib.hypo_gpu_kset_query_depth(_p(buf), _p(off), C.c_uint32(n), C.c_uint32(bin), C.c_uint32(text), C.c_uint32(unit), C.c_uint64(n_bins),
                                                    *[_p(a) for a in u32], _p(med)))
        return (rc,) + tuple(a[:n_bins] for a in u32) + (med[:n_bins],)

    def kset_query_depth(self, seqs_or_text, off=None, bin=1024, text=0, unit=1):
        """per bin of `bin` window starts of every sequence (bins numbered sequence by sequence): (windows, missing, rated, over,
        under, med_count) of the read count bytes against the copy bytes of plane `text`, a copy being worth `unit` reads"""
        out = self.kset_query_depth_rc(seqs_or_text, off, bin, text, unit)
        self._check(out[0])
        return out[1:]

    def kset_export_rc(self, cursor: int, cap: int, keys, counts=None):
        """(return code, cursor after the call, n_out, digest of the call) of ONE call of hypo_gpu_kset_export into the caller's arrays:
        keys u64[>= cap], counts u8[>= cap] or None; nothing is checked here.  n_out is None when the call did not write it."""
        untouched = 0xFFFFFFFFFFFFFFFF                                  # (no call hands back 2^64 - 1 records)
        cur, n_out, dig = C.c_uint64(cursor), C.c_uint64(untouched), C.c_uint64(0)
        rc = int(self.lib.hypo_gpu_kset_export(C.byref(cur), _p(keys), _p(counts) if counts is not None else None, C.c_uint64(cap), C.byref(n_out), C.byref(dig)))
        return rc, int(cur.value), None if n_out.value == untouched else int(n_out.value), int(dig.value)

    def kset_export(self, cap: int = 1 << 20, counts=True):
        """one export sequence over the set with calls of `cap`: (keys u64[n], counts u8[n] or None, digest, the n_out of every call)"""
        n = self.kset_size()[0]
        keys = np.empty(n + cap, np.uint64)                              # (room for a whole call behind the last record)
        cnts = np.empty(n + cap, np.uint8) if counts else None
        cursor, at, digest, n_outs = 0, 0, 0, []
        while cursor != abi.KSET_EXPORT_END:
            rc, cursor, got, d = self.kset_export_rc(cursor, cap, keys[at:], cnts[at:] if counts else None)
            self._check(rc)
            at += got
            digest = (digest + d) & 0xFFFFFFFFFFFFFFFF
            n_outs.append(got)
        return keys[:at], cnts[:at] if counts else None, digest, n_outs

    def kset_import_rc(self, keys, counts=None):
        """(return code, digest of the records as given) of one call of hypo_gpu_kset_import; nothing is checked here"""
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        n = keys.size
        pad = lambda x, t: np.concatenate([x, np.zeros(1, t)])          # (an empty array still has an address)
        if counts is not None:
            counts = np.ascontiguousarray(counts, dtype=np.uint8)
            assert counts.size == n
        dig = C.c_uint64(0)
        rc = int(self.lib.hypo_gpu_kset_import(_p(pad(keys, np.uint64)), _p(pad(counts, np.uint8)) if counts is not None else None, C.c_uint64(n), C.byref(dig)))
        return rc, int(dig.value)

    def kset_import(self, keys, counts=None) -> int:
        """every key into the set, its count byte going up by counts[i] (None: 1 each) and stopping at 255; the digest of the records"""
        rc, dig = self.kset_import_rc(keys, counts)
        self._check(rc)
        return dig

    def kset_end(self):
        self._check(self.lib.hypo_gpu_kset_end())

    def _solid_build_files(self, paths, k, coverage):
        from .host import LIB_PATH as HOST_LIB
        host = C.CDLL(HOST_LIB)
        arr = (C.c_char_p * len(paths))(*[p.encode() for p in paths])
        words = np.zeros((1 << (2 * k)) // 64, dtype=np.uint64)
        hist = np.zeros(4 * coverage + 1, dtype=np.uint64)
        cut = (C.c_uint32 * 4)()
        counts = (C.c_uint64 * 4)()
        times = (C.c_double * 5)()
        err = C.create_string_buffer(512)
        rc = host.hypo_host_solid_build(arr, C.c_int(len(paths)), C.c_uint32(k), C.c_uint32(coverage), _p(words), _p(hist),
                                        cut, counts, times, err, C.c_int(512))
        if rc == 2:
            return {"hist": hist, "cut": None}
        if rc != 0:
            raise HypoGpuError(f"solid k-mer construction failed (rc={rc}): {err.value.decode()}")
        return {"hist": hist, "cut": tuple(int(x) for x in cut), "bits": words, "n_bits": int(counts[0]),
                "n_canonical": int(counts[1]), "seq_bytes": int(counts[2]), "file_bytes": int(counts[3]),
                "times": tuple(float(x) for x in times)}

    def solid_scan(self, packed4: np.ndarray, n_bases: int, k: int, bits: np.ndarray, kids_cap=None):
        nw = (n_bases + 63) // 64
        words = np.zeros(max(nw, 1), dtype=np.uint64)
        if kids_cap is None:
            kids_cap = n_bases
        kids = np.zeros(max(kids_cap, 1), dtype=np.uint64)
        rank = np.zeros(nw + 1, dtype=np.uint64)
        ns = C.c_uint64(0)
        self._check(self.lib.hypo_gpu_solid_scan(_p(packed4), C.c_uint64(n_bases), C.c_uint32(k), _p(bits),
                                                 _p(words), _p(kids), C.c_uint64(kids_cap), _p(rank),
                                                 C.byref(ns)))
        n = int(ns.value)
        return words[:nw], kids[:min(n, kids_cap)], rank, n

    # ---- HIP-event kernel timing --------------------------------------------------------------------------
    def profile_begin(self, max_calls: int):
        self._check(self.lib.hypo_gpu_profile_begin(C.c_int(max_calls)))

    def profile_read(self):
        """List of per-call lists of elapsed milliseconds (see include/hypo_gpu.h)."""
        out = []
        buf = (C.c_float * 16)()
        for c in range(int(self.lib.hypo_gpu_profile_calls())):
            n = int(self.lib.hypo_gpu_profile_read(C.c_int(c), buf, C.c_int(16)))
            if n < 0:
                self._check(n)
            out.append([float(buf[i]) for i in range(n)])
        return out

    # ---- device-resident entry points (torch tensors own the HBM) --------------------------------------
    def device_batch(self, b: HostBatch, off=None, workspace_bytes=None):
        """workspace_bytes: None = the size hypo_gpu_poa_workspace_bytes recommends"""
        return DeviceBatch(self, b, off, workspace_bytes)

    def device_scan(self, packed4: np.ndarray, n_bases: int, k: int, bits: np.ndarray, kids_cap=None, misalign=0):
        return DeviceScan(self, packed4, n_bases, k, bits, kids_cap, misalign)


def _stats_dict(s: abi.PoaStats) -> dict:
    return {"n_windows": int(s.n_windows), "n_trivial": int(s.n_trivial),
            "n_class": [int(x) for x in s.n_class], "n_escalated": int(s.n_escalated),
            "n_failed": int(s.n_failed), "dp_cells": int(s.dp_cells), "n_alignments": int(s.n_alignments),
            "alg_bytes": [int(x) for x in s.alg_bytes], "n_reused": int(s.n_reused), "n_threaded": int(s.n_threaded),
            "cells_scored": int(s.cells_scored), "cells_threaded": int(s.cells_threaded), "n_carried": int(s.n_carried)}


def _t(arr, dev):
    import torch
    a = np.ascontiguousarray(arr)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    elif a.dtype.fields is not None:
        a = a.view(np.uint8)
    if a.size == 0:
        return torch.zeros(16, dtype=torch.uint8, device=dev)
    return torch.from_numpy(a).to(dev)


class DeviceBatch:
    """A window batch resident in HBM + its output buffers and workspace (torch owns the memory)."""

    def __init__(self, gpu: HypoGpu, b: HostBatch, off=None, workspace_bytes=None):
        import torch
        self.gpu, self.host = gpu, b
        dev = torch.device("cuda", gpu.device)
        self.dev = dev
        n = b.n_windows
        if off is None:
            off = b.slot_layout()
        self.off_host = off
        self.windows = _t(b.windows, dev)
        self.draft4, self.arm_off, self.arm_len, self.arms2 = (_t(x, dev) for x in (b.draft4, b.arm_off, b.arm_len, b.arms2))
        self.off = _t(off, dev)
        self.bases = torch.zeros(int(off[-1]) + 16, dtype=torch.uint8, device=dev)
        self.len = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
        self.status = torch.zeros(max(n, 1), dtype=torch.uint8, device=dev)
        wsb = int(gpu.lib.hypo_gpu_poa_workspace_bytes(C.c_uint32(n), C.c_uint32(b.n_arms)))
        if workspace_bytes is not None:
            wsb = int(workspace_bytes)
        self.workspace = torch.zeros(wsb, dtype=torch.uint8, device=dev)
        s = abi.WindowBatch()
        s.n_windows, s.n_arms = n, b.n_arms
        s.windows, s.draft4, s.draft4_bytes = self.windows.data_ptr(), self.draft4.data_ptr(), b.draft4.size
        s.arm_off, s.arm_len = self.arm_off.data_ptr(), self.arm_len.data_ptr()
        s.arms2, s.arms2_bytes = self.arms2.data_ptr(), b.arms2.size
        self.in_struct = s
        self.out_struct = abi.ConsensusBatch(self.bases.data_ptr(), self.off.data_ptr(), self.len.data_ptr(),
                                             self.status.data_ptr())

    def run(self, scores=abi.DEFAULT_SCORES, stream=None):
        """Enqueues the whole POA of the batch on `stream` (torch current stream by default); asynchronous."""
        import torch
        sp = abi.ScoreParams(*scores)
        st = stream if stream is not None else torch.cuda.current_stream(self.dev)
        self.gpu._check(self.gpu.lib.hypo_gpu_poa_batch_device(
            C.byref(sp), C.byref(self.in_struct), C.byref(self.out_struct),
            C.c_void_p(self.workspace.data_ptr()), C.c_size_t(self.workspace.numel()),
            C.c_void_p(st.cuda_stream)))

    def stats(self, stream=None) -> dict:
        import torch
        st = stream if stream is not None else torch.cuda.current_stream(self.dev)
        s = abi.PoaStats()
        self.gpu._check(self.gpu.lib.hypo_gpu_poa_read_stats(C.c_void_p(self.workspace.data_ptr()),
                                                             C.c_void_p(st.cuda_stream), C.byref(s)))
        d = _stats_dict(s)
        d["n_windows"] = self.host.n_windows
        return d

    def results(self):
        """(bases u8, off u64, len u32, status u8) copied back to the host."""
        import torch
        torch.cuda.synchronize(self.dev)
        n = self.host.n_windows
        return (self.bases.cpu().numpy(), self.off_host, self.len.cpu().numpy().view(np.uint32)[:n],
                self.status.cpu().numpy()[:n])

    def consensus(self):
        bases, off, ln, st = self.results()
        return [bases[int(off[i]):int(off[i]) + int(ln[i])].tobytes().decode() if st[i] == 0 else None
                for i in range(self.host.n_windows)], st


class DeviceScan:
    """A contig + solid-kmer set resident in HBM and the scan outputs."""

    def __init__(self, gpu: HypoGpu, packed4: np.ndarray, n_bases: int, k: int, bits: np.ndarray, kids_cap=None, misalign=0):
        import torch
        self.gpu, self.n_bases, self.k = gpu, n_bases, k
        dev = torch.device("cuda", gpu.device)
        self.dev = dev
        self.nw = (n_bases + 63) // 64
        self.kids_cap = n_bases if kids_cap is None else kids_cap
        self.packed4, self.bits = _t(packed4, dev), _t(bits, dev)
        if misalign:                 # the contig at an address that is not a multiple of 8 (a view into a larger buffer)
            self._backing = torch.zeros(self.packed4.numel() + misalign, dtype=torch.uint8, device=dev)
            self._backing[misalign:] = self.packed4
            self.packed4 = self._backing[misalign:]
        self.words = torch.zeros(max(self.nw, 1), dtype=torch.int64, device=dev)
        self.kids = torch.zeros(max(self.kids_cap, 1), dtype=torch.int64, device=dev)
        self.rank = torch.zeros(self.nw + 1, dtype=torch.int64, device=dev)
        self.n_solid = torch.zeros(1, dtype=torch.int64, device=dev)
        wsb = int(gpu.lib.hypo_gpu_solid_scan_workspace_bytes(C.c_uint64(n_bases)))
        self.workspace = torch.zeros(wsb, dtype=torch.uint8, device=dev)

    def run(self, stream=None):
        import torch
        st = stream if stream is not None else torch.cuda.current_stream(self.dev)
        self.gpu._check(self.gpu.lib.hypo_gpu_solid_scan_device(
            C.c_void_p(self.packed4.data_ptr()), C.c_uint64(self.n_bases), C.c_uint32(self.k),
            C.c_void_p(self.bits.data_ptr()), C.c_void_p(self.words.data_ptr()),
            C.c_void_p(self.kids.data_ptr()), C.c_uint64(self.kids_cap), C.c_void_p(self.rank.data_ptr()),
            C.c_void_p(self.n_solid.data_ptr()), C.c_void_p(self.workspace.data_ptr()),
            C.c_size_t(self.workspace.numel()), C.c_void_p(st.cuda_stream)))

    def results(self):
        import torch
        torch.cuda.synchronize(self.dev)
        n = int(self.n_solid.item())
        return (self.words.cpu().numpy().view(np.uint64)[:self.nw],
                self.kids.cpu().numpy().view(np.uint64)[:min(n, self.kids_cap)],
                self.rank.cpu().numpy().view(np.uint64), n)
