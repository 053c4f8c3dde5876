"""fastkmer_amd -- MI355X-native exact k-mer counter (host-side mirror).

The compute path is the HIP library ``fastkmer_amd/lib/libfastkmer.so``
(C-ABI in ``include/fastkmer.h``); this module binds it with ctypes and
mirrors the reference's driver-side API:

* :class:`TestConfiguration`  -- skc.test.testutil.TestConfiguration
  (src/main/scala/skc/test/package.scala:16-42)
* :func:`execute_job`         -- SparkBinKmerCounter.executeJob
  (src/main/scala/skc/SparkBinKmerCounter.scala:989-1046)
* :class:`KmerCounter`        -- the map / shuffle / reduce hot path as one
  device-resident object (getSuperKmers :34-169, reduceByKey :1035,
  extractKXmers :428-660, extractKXmersHT :664-739)

There is no CPU fallback: without the built library, or without a GPU,
constructing a :class:`KmerCounter` raises.
"""
from __future__ import annotations

import ctypes
import dataclasses
import os
import re

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FASTKMER_LIB") or os.path.join(_PKG, "lib", "libfastkmer.so")
CLI_PATH = os.path.join(_PKG, "bin", "fastkmer-cli")
HEADER_PATH = os.path.join(os.path.dirname(_PKG), "include", "fastkmer.h")

FK_OK = 0
ERRORS = {-1: "FK_E_INVALID", -2: "FK_E_STATE", -3: "FK_E_DEVICE", -4: "FK_E_NOMEM", -5: "FK_E_IO",
          -6: "FK_E_RANGE", -7: "FK_E_COMM"}
ABI_VERSION = 3  # include/fastkmer.h FK_ABI_VERSION this binding mirrors (fk_config / fk_stats layouts)


class FastKmerError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"{ERRORS.get(code, code)}: {message}")
        self.code = code


class fk_config(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in
                ("k", "m", "x", "B", "use_ht", "sequence_type", "write", "n_ranks", "rank", "device")]


class fk_stats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in
                ("fasta_bytes", "positions", "bases", "kmers", "superkmers", "records_received", "distinct",
                 "oversize_buckets", "buckets", "fine_bits")] + \
               [(n, ctypes.c_double) for n in
                ("ms_parse", "ms_signature", "ms_partition", "ms_count", "ms_total", "ms_encode_kernel",
                 "ms_signature_kernel")] + [("fused_map", ctypes.c_uint64), ("ms_h2d", ctypes.c_double),
                                       ("fused_fallback", ctypes.c_uint64),
                                       ("xch_steps", ctypes.c_uint64), ("xch_bytes_sent", ctypes.c_uint64),
                                       ("xch_bytes_received", ctypes.c_uint64), ("ms_exchange", ctypes.c_double),
                                       ("ms_exchange_tail", ctypes.c_double),
                                       ("pieces_counted", ctypes.c_uint64),
                                       ("heavy_keys", ctypes.c_uint64), ("block_buckets", ctypes.c_uint64), ("big_buckets", ctypes.c_uint64),
                                       ("split_buckets", ctypes.c_uint64),
                                       ("sub_buckets", ctypes.c_uint64)]


class fk_db_info(ctypes.Structure):
    """Mirror of fk_db_info (include/fastkmer.h): the header of a database file."""
    _fields_ = [(n, ctypes.c_int32) for n in
                ("k", "m", "bins", "key_words", "n_ranks", "rank", "version", "stored_bins")] + \
               [(n, ctypes.c_uint64) for n in ("distinct", "kmers", "checksum", "file_bytes")]


class fk_read_stat(ctypes.Structure):
    """Mirror of fk_read_stat (include/fastkmer.h): one read's statistics, 32 bytes."""
    _fields_ = [(n, ctypes.c_uint32) for n in ("windows", "hits", "min", "median", "max", "reserved")] + \
               [("sum", ctypes.c_uint64)]


READ_STAT_DTYPE = np.dtype([(n, np.uint32) for n in ("windows", "hits", "min", "median", "max", "reserved")] +
                           [("sum", np.uint64)])  # the numpy view of fk_read_stat
READ_TILE = 4096  # FK_READ_TILE: positions per workgroup tile of the window kernel

COMM_ID_BYTES = 128
MAX_COUNT = 0xFFFFFFFF  # max_count of the count-range calls: no upper bound


def _count_range(min_count, max_count):
    """(lo, hi) of a count range for the C calls, or None for the default (every k-mer)."""
    hi = MAX_COUNT if max_count is None else int(max_count)
    lo = int(min_count)
    if not (0 <= lo <= MAX_COUNT and 0 <= hi <= MAX_COUNT):
        raise ValueError("min_count / max_count are 32-bit counts")
    return None if (lo, hi) == (1, MAX_COUNT) else (lo, hi)


_lib = None


def header_functions() -> list[str]:
    """Names of the functions declared in include/fastkmer.h."""
    with open(HEADER_PATH) as f:
        text = f.read()
    return re.findall(r"^[A-Za-z_][\w \*]*?\b(fk_\w+)\s*\(", text, re.M)


def lib():
    """Load the HIP library (raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: build it with `python -m fastkmer_amd.build` "
                           "(there is no CPU fallback)")
    # One HIP runtime per process: torch ships its own libamdhip64 with the
    # same SONAME as /opt/rocm's.  Loading torch first makes the dynamic
    # loader bind libfastkmer.so to that runtime, so device pointers, streams
    # and RCCL (torch.distributed "nccl") are shared with torch.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(LIB_PATH)
    P, I32, U64, SZ = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint64, ctypes.c_size_t
    sig = {
        "fk_abi_version": (ctypes.c_int, []),
        "fk_config_init": (ctypes.c_int, [ctypes.POINTER(fk_config)]),
        "fk_config_validate": (ctypes.c_int, [ctypes.POINTER(fk_config)]),
        "fk_clamped_bins": (I32, [I32, I32]),
        "fk_output_dir": (ctypes.c_int, [ctypes.POINTER(fk_config), ctypes.c_char_p, ctypes.c_char_p,
                                         ctypes.c_char_p, SZ]),
        "fk_record_bytes_for_k": (SZ, [I32]),
        "fk_synth_record_bytes": (U64, [I32]),
        "fk_synth_fasta_host": (ctypes.c_int, [P, U64, U64, I32, U64, U64, ctypes.c_double, ctypes.c_double]),
        "fk_create": (ctypes.c_int, [ctypes.POINTER(fk_config), ctypes.POINTER(P)]),
        "fk_destroy": (None, [P]),
        "fk_last_error": (ctypes.c_char_p, []),
        "fk_set_stream": (ctypes.c_int, [P, P]),
        "fk_ingest": (ctypes.c_int, [P, ctypes.c_char_p, SZ, ctypes.c_int]),
        "fk_ingest_device": (ctypes.c_int, [P, P, SZ, ctypes.c_int]),
        "fk_ingest_reserve": (ctypes.c_int, [P, U64]),
        "fk_split_bytes": (ctypes.c_int, [ctypes.c_char_p, I32, I32, I32, I32, P, SZ, ctypes.POINTER(SZ)]),
        "fk_ingest_file_range": (ctypes.c_int, [P, ctypes.c_char_p, I32, I32, U64]),
        "fk_set_input_format": (ctypes.c_int, [P, I32, I32, I32]),
        "fk_input_format": (ctypes.c_int, [P, ctypes.POINTER(I32), ctypes.POINTER(I32), ctypes.POINTER(I32)]),
        "fk_fastq_info": (ctypes.c_int, [P, P]),
        "fk_debug_fastq_ms": (ctypes.c_int, [P, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(U64)]),
        "fk_fastq_frontier": (ctypes.c_int, [ctypes.c_char_p, SZ, ctypes.POINTER(SZ)]),
        "fk_split_bytes_fastq": (ctypes.c_int, [ctypes.c_char_p, I32, I32, P, SZ, ctypes.POINTER(SZ)]),
        "fk_synth_fasta_device": (ctypes.c_int, [P, U64, U64, I32, U64, U64, ctypes.c_double, ctypes.c_double]),
        "fk_synth_fasta_to_device": (ctypes.c_int, [P, U64, U64, I32, U64, U64, ctypes.c_double, ctypes.c_double]),
        "fk_map": (ctypes.c_int, [P, P]),
        "fk_record_bytes": (SZ, [P]),
        "fk_map_emit": (ctypes.c_int, [P, P, U64]),
        "fk_reduce": (ctypes.c_int, [P, P, U64]),
        "fk_set_grouped_emit": (ctypes.c_int, [P, ctypes.c_int32]),
        "fk_grouped_parts_per_rank": (ctypes.c_int32, [P]),
        "fk_map_part_counts": (ctypes.c_int, [P, P, P]),
        "fk_reduce_grouped": (ctypes.c_int, [P, P, U64, P, P, ctypes.c_int32, ctypes.c_int32]),
        "fk_finish": (ctypes.c_int, [P]),
        "fk_num_bins": (I32, [P]),
        "fk_bin_sizes": (ctypes.c_int, [P, P]),
        "fk_get_bin": (ctypes.c_int, [P, I32, P, P, SZ, ctypes.POINTER(SZ)]),
        "fk_write_bins": (ctypes.c_int, [P, ctypes.c_char_p]),
        "fk_get_stats": (ctypes.c_int, [P, ctypes.POINTER(fk_stats)]),
        "fk_kmer_bin": (ctypes.c_int, [ctypes.POINTER(fk_config), P, P]),
        "fk_query": (ctypes.c_int, [P, P, SZ, P, P]),
        "fk_query_device": (ctypes.c_int, [P, P, SZ, P, P]),
        "fk_query_sequence": (ctypes.c_int, [P, ctypes.c_char_p, SZ, P, SZ, ctypes.POINTER(SZ)]),
        "fk_reads_csr": (ctypes.c_int, [ctypes.c_char_p, SZ, I32, I32, I32, P, SZ, P, SZ, ctypes.POINTER(SZ),
                                        ctypes.POINTER(SZ)]),
        "fk_read_counts_device": (ctypes.c_int, [P, P, P, SZ, P, P]),
        "fk_read_counts": (ctypes.c_int, [P, P, P, SZ, P, P]),
        "fk_read_stats_of_counts_device": (ctypes.c_int, [P, P, P, P, SZ, ctypes.c_uint32, ctypes.c_uint32, P]),
        "fk_read_stats_device": (ctypes.c_int, [P, P, P, SZ, ctypes.c_uint32, ctypes.c_uint32, P, SZ, P]),
        "fk_read_stats": (ctypes.c_int, [P, P, P, SZ, ctypes.c_uint32, ctypes.c_uint32, P]),
        "fk_read_stats_scratch_bytes": (SZ, [SZ]),
        "fk_spectrum": (ctypes.c_int, [P, P, SZ, P]),
        "fk_spectrum_device": (ctypes.c_int, [P, P, SZ, P]),
        "fk_bin_sizes_range": (ctypes.c_int, [P, ctypes.c_uint32, ctypes.c_uint32, P]),
        "fk_get_bin_range": (ctypes.c_int, [P, I32, ctypes.c_uint32, ctypes.c_uint32, P, P, SZ,
                                            ctypes.POINTER(SZ)]),
        "fk_write_bins_range": (ctypes.c_int, [P, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32]),
        "fk_compare": (ctypes.c_int, [P, P, P, SZ, SZ]),
        "fk_compare_device": (ctypes.c_int, [P, P, P, SZ, SZ]),
        "fk_bin_sizes_joined": (ctypes.c_int, [P, P, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                               ctypes.c_uint32, P]),
        "fk_get_bin_joined": (ctypes.c_int, [P, P, I32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                             ctypes.c_uint32, P, P, P, SZ, ctypes.POINTER(SZ)]),
        "fk_export": (ctypes.c_int, [P, P, P, SZ, ctypes.POINTER(SZ)]),
        "fk_export_device": (ctypes.c_int, [P, P, P, SZ, ctypes.POINTER(SZ)]),
        "fk_import": (ctypes.c_int, [P, P, P, P]),
        "fk_import_device": (ctypes.c_int, [P, P, P, P]),
        "fk_db_info_read": (ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(fk_db_info)]),
        "fk_save": (ctypes.c_int, [P, ctypes.c_char_p]),
        "fk_load": (ctypes.c_int, [P, ctypes.c_char_p]),
        "fk_debug_store_ms": (ctypes.c_int, [P, P]),
        "fk_map_bin_kmers": (ctypes.c_int, [P, P]),
        "fk_lpt_owners": (ctypes.c_int, [P, I32, I32, P]),
        "fk_set_bin_owners": (ctypes.c_int, [P, P, P]),
        "fk_bin_owners": (ctypes.c_int, [P, P]),
        "fk_signature_slots": (U64, [P]),
        "fk_signature_counts": (ctypes.c_int, [P, P, U64]),
        "fk_write_bin_signatures": (ctypes.c_int, [P, P, U64, ctypes.c_char_p]),
        "fk_find_bin_signatures": (ctypes.c_int, [P, ctypes.c_char_p]),
        "fk_comm_unique_id": (ctypes.c_int, [P]),
        "fk_comm_init": (ctypes.c_int, [P, P]),
        "fk_comm_init_local": (ctypes.c_int, [P, I32]),
        "fk_comm_transport": (ctypes.c_char_p, [P]),
        "fk_comm_allreduce_u64": (ctypes.c_int, [P, P, SZ]),
        "fk_balance_bins": (ctypes.c_int, [P, ctypes.c_char_p, SZ]),
        "fk_balance_bins_file": (ctypes.c_int, [P, ctypes.c_char_p, I32, I32, ctypes.c_double]),
        "fk_exchange_plan": (ctypes.c_int, [I32, I32, P, P, U64, P, P, P, P, P]),
        "fk_debug_map_cycles": (ctypes.c_int, [P, I32]),
        "fk_debug_comm_hold": (ctypes.c_int, [P, I32]),
        "fk_debug_comm_release": (ctypes.c_int, [P]),
        "fk_debug_comm_held": (ctypes.c_int, [P]),
        "fk_debug_fingerprint_bits": (ctypes.c_int, [I32, I32]),
        "fk_debug_wave_count": (ctypes.c_int, [I32, I32, I32, ctypes.c_uint32, ctypes.c_uint32, I32, P,
                                               ctypes.c_uint32, P, P, P]),
        "fk_debug_wave_count_w": (ctypes.c_int, [I32, I32, I32, ctypes.c_uint32, ctypes.c_uint32, I32, P,
                                                 ctypes.c_uint32, P, P, P]),
        "fk_debug_fold_stats": (ctypes.c_int, [P, P]),
        "fk_debug_count_pieces": (ctypes.c_int, [P, I32, I32, P, P, I32, ctypes.c_uint32]),
        "fk_debug_tier_stats": (ctypes.c_int, [P, P]),
        "fk_debug_staged_piece": (ctypes.c_int, [P, I32, P, P]),
        "fk_debug_live_resources": (ctypes.c_int, [P]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    if L.fk_abi_version() != ABI_VERSION:
        raise RuntimeError(f"{LIB_PATH} has ABI version {L.fk_abi_version()}, this binding mirrors {ABI_VERSION}: "
                           "rebuild it (python -m fastkmer_amd.build)")
    _lib = L
    return L


def _check(rc: int) -> None:
    if rc != FK_OK:
        raise FastKmerError(rc, lib().fk_last_error().decode(errors="replace"))


def make_config(k: int, m: int, x: int = 3, B: int = 2048, use_ht: bool = False, sequence_type: int = 0,
                write: bool = False, n_ranks: int = 1, rank: int = 0, device: int = -1) -> fk_config:
    c = fk_config()
    lib().fk_config_init(ctypes.byref(c))
    c.k, c.m, c.x, c.B = k, m, x, B
    c.use_ht, c.sequence_type, c.write = int(bool(use_ht)), sequence_type, int(bool(write))
    c.n_ranks, c.rank, c.device = n_ranks, rank, device
    return c


def validate(**kw) -> None:
    """Host-only configuration check (no GPU); raises FastKmerError."""
    c = make_config(**kw)
    _check(lib().fk_config_validate(ctypes.byref(c)))


def clamped_bins(m: int, B: int) -> int:
    return lib().fk_clamped_bins(m, B)


def record_bytes_for_k(k: int) -> int:
    return lib().fk_record_bytes_for_k(k)


def synth_fasta(n_reads: int, read_len: int = 100, genome_len: int = 1_000_000, seed: int = 0x5EED,
                err_rate: float = 0.002, n_rate: float = 0.0005, first_read: int = 0) -> bytes:
    """Deterministic synthetic short-read FASTA (byte-identical to the device generator)."""
    L = lib()
    nb = n_reads * L.fk_synth_record_bytes(read_len)
    buf = ctypes.create_string_buffer(max(nb, 1))
    _check(L.fk_synth_fasta_host(buf, first_read, n_reads, read_len, genome_len, seed, err_rate, n_rate))
    return buf.raw[:nb]


def synth_fasta_to_device(ptr: int, n_reads: int, read_len: int = 100, genome_len: int = 1_000_000,
                          seed: int = 0x5EED, err_rate: float = 0.002, n_rate: float = 0.0005,
                          first_read: int = 0) -> int:
    """The bytes of synth_fasta written into a device buffer at ptr (current device); returns the size."""
    L = lib()
    _check(L.fk_synth_fasta_to_device(ctypes.c_void_p(ptr), first_read, n_reads, read_len, genome_len, seed,
                                      err_rate, n_rate))
    return n_reads * L.fk_synth_record_bytes(read_len)


def split_bytes(path: str, world: int, rank: int, k: int, sequence_type: int = 0) -> bytes:
    """The bytes rank `rank` of `world` ingests from the FASTA file at `path` (fk_split_bytes: the
    FASTdoop-style input split of SBKC:993, 1009-1012; host only)."""
    L = lib()
    n = ctypes.c_size_t()
    p = os.fsencode(path)
    _check(L.fk_split_bytes(p, world, rank, k, sequence_type, None, 0, ctypes.byref(n)))
    buf = ctypes.create_string_buffer(max(n.value, 1))
    _check(L.fk_split_bytes(p, world, rank, k, sequence_type, buf, n.value, ctypes.byref(n)))
    return buf.raw[:n.value]


FORMATS = {"fasta": 0, "fastq": 1}  # FK_FORMAT_*


def split_bytes_fastq(path: str, world: int, rank: int) -> bytes:
    """The bytes rank `rank` of `world` ingests from the FASTQ file at `path` (fk_split_bytes_fastq:
    the whole records whose '@' line starts in the rank's byte range; host only)."""
    L = lib()
    n = ctypes.c_size_t()
    p = os.fsencode(path)
    _check(L.fk_split_bytes_fastq(p, world, rank, None, 0, ctypes.byref(n)))
    buf = ctypes.create_string_buffer(max(n.value, 1))
    _check(L.fk_split_bytes_fastq(p, world, rank, buf, n.value, ctypes.byref(n)))
    return buf.raw[:n.value]


def fastq_frontier(buf: bytes) -> int:
    """fk_fastq_frontier: the start of the last FASTQ record of buf whose '@' line and '+' line both
    begin inside it (buf[0] counts as a line start); len(buf) when there is none.  Host only."""
    raw = bytes(buf)
    off = ctypes.c_size_t()
    _check(lib().fk_fastq_frontier(raw, len(raw), ctypes.byref(off)))
    return off.value


def reads_csr(text, input_format: str = "fasta", min_quality: int = 0, quality_offset: int = 33):
    """fk_reads_csr: FASTA / FASTQ text cut into a CSR read batch as the count sees it -- (bases, offsets):
    uint8[n_bases] sequence bytes back to back, uint64[n_reads + 1] ascending from 0 to n_bases.  Host only.
    FastKmerError (FK_E_INVALID) naming the first malformed FASTQ record."""
    if input_format not in FORMATS:
        raise ValueError(f"input_format must be one of {sorted(FORMATS)}")
    raw = text.encode() if isinstance(text, str) else bytes(text)
    L = lib()
    nr, nb = ctypes.c_size_t(), ctypes.c_size_t()
    args = (raw, len(raw), FORMATS[input_format], int(min_quality), int(quality_offset))
    _check(L.fk_reads_csr(*args, None, 0, None, 0, ctypes.byref(nr), ctypes.byref(nb)))
    bases = np.zeros(nb.value, dtype=np.uint8)
    offsets = np.zeros(nr.value + 1, dtype=np.uint64)
    _check(L.fk_reads_csr(*args, bases.ctypes.data, bases.size, offsets.ctypes.data, nr.value, ctypes.byref(nr),
                          ctypes.byref(nb)))
    return bases, offsets


def db_info(path: str) -> dict:
    """fk_db_info_read: the validated header of a database file written by KmerCounter.save -- k, m, bins,
    key_words, n_ranks, rank, version, stored_bins, distinct, kmers, checksum, file_bytes.  Host only.
    FastKmerError: FK_E_INVALID for bytes that are no header of this version, FK_E_IO for a file that
    cannot be read or whose size is not the one its header gives."""
    h = fk_db_info()
    _check(lib().fk_db_info_read(os.fsencode(path), ctypes.byref(h)))
    return {n: int(getattr(h, n)) for n, _ in fk_db_info._fields_}


def read_stats_scratch_bytes(n_bases: int) -> int:
    """fk_read_stats_scratch_bytes: the scratch read_stats_ptr needs for a batch of n_bases bases."""
    return lib().fk_read_stats_scratch_bytes(int(n_bases))


def filter_reads(stats, min_hits: int = 0, max_hits: int | None = None) -> np.ndarray:
    """kmc_tools filter on read statistics: the bool mask of the reads whose number of k-mers with a count
    in the range the statistics were made with (stats["hits"]) lies in [min_hits, max_hits], both ends
    inclusive (max_hits None: no upper bound)."""
    hits = np.asarray(stats)["hits"]
    keep = hits >= min_hits
    if max_hits is not None:
        keep &= hits <= max_hits
    return keep


def _csr_arrays(bases, offsets):
    if isinstance(bases, (bytes, bytearray, str)):
        bases = np.frombuffer(bases.encode() if isinstance(bases, str) else bytes(bases), dtype=np.uint8)
    b = np.ascontiguousarray(bases, dtype=np.uint8).reshape(-1)
    o = np.ascontiguousarray(offsets, dtype=np.uint64).reshape(-1)
    if o.size < 1:
        raise ValueError("offsets has n_reads + 1 entries")
    if int(o[-1]) != b.size:
        raise ValueError(f"offsets ends at {int(o[-1])}, bases holds {b.size}")
    return b, o


def decode_keys(keys: np.ndarray, k: int) -> list[str]:
    """2-bit keys (one word for k <= 32, (hi, lo) pairs for k > 32) -> strings."""
    out = []
    words = keys.reshape(-1, 2) if k > 32 else keys.reshape(-1, 1)
    for row in words:
        v = (int(row[0]) << 64) | int(row[1]) if k > 32 else int(row[0])
        s = []
        for _ in range(k):
            s.append("ACGT"[v & 3])
            v >>= 2
        out.append("".join(reversed(s)))
    return out


def encode_keys(kmers: list[str], k: int) -> np.ndarray:
    """Strings -> 2-bit keys in get_bin's layout (the inverse of decode_keys): one uint64 per k-mer
    for k <= 32, (hi, lo) pairs (a flat array) for k > 32.  ValueError on a character other than
    A/C/G/T or a string whose length is not k."""
    kw = 2 if k > 32 else 1
    out = np.zeros(len(kmers) * kw, dtype=np.uint64)
    code = {"A": 0, "C": 1, "G": 2, "T": 3}
    for i, s in enumerate(kmers):
        if len(s) != k:
            raise ValueError(f"k-mer {i} has {len(s)} characters, k = {k}")
        v = 0
        for ch in s:
            if ch not in code:
                raise ValueError(f"k-mer {i} holds {ch!r}: only A, C, G, T")
            v = (v << 2) | code[ch]
        if kw == 2:
            out[2 * i], out[2 * i + 1] = v >> 64, v & 0xFFFFFFFFFFFFFFFF
        else:
            out[i] = v
    return out


def kmer_bin(key_or_str, k: int, m: int, B: int) -> int:
    """The bin of a k-mer (a string, or a key in get_bin's layout: an int / one uint64 for k <= 32,
    (hi, lo) for k > 32; either strand) under (k, m, B) -- fk_kmer_bin, host only."""
    if isinstance(key_or_str, str):
        key = encode_keys([key_or_str], k)
    else:
        key = np.ascontiguousarray(key_or_str, dtype=np.uint64).reshape(-1)
    if key.size != (2 if k > 32 else 1):
        raise ValueError(f"a key for k = {k} has {2 if k > 32 else 1} word(s)")
    cfg = make_config(k, m, 1, B)
    b = ctypes.c_int32(-1)
    _check(lib().fk_kmer_bin(ctypes.byref(cfg), key.ctypes.data, ctypes.byref(b)))
    return b.value


@dataclasses.dataclass
class TestConfiguration:
    """Mirror of skc.test.testutil.TestConfiguration (test/package.scala:16-42)."""
    __test__ = False  # not a pytest class

    dataset: str
    outputDirectory: str
    k: int
    m: int
    x: int
    max_b: int = 2000
    sequenceType: int = 0
    canonical: bool = True
    debug: bool = False
    write: bool = True
    useKryoSerializer: bool = False
    useHT: bool = False
    useCustomPartitioner: bool = False
    numPartitionTasks: int = 0
    prefix: str = ""

    @property
    def b(self) -> int:  # :32
        return int(min(4.0 ** self.m, float(self.max_b)))

    @property
    def outputDir(self) -> str:  # :33
        base = "/tmp/" if self.debug else self.outputDirectory
        tail = f"{self.prefix}k{self.k}_m{self.m}_x{self.x}_b{self.b}"
        return base + tail if self.debug else base + tail + f"_s{self.sequenceType}"


class KmerCounter:
    """Device-resident exact canonical k-mer counter for one rank."""

    def __init__(self, k: int, m: int, x: int = 3, B: int = 2048, use_ht: bool = False, sequence_type: int = 0,
                 n_ranks: int = 1, rank: int = 0, device: int = -1, input_format: str = "fasta",
                 min_quality: int = 0, quality_offset: int = 33):
        L = lib()
        if input_format not in FORMATS:
            raise ValueError(f"input_format must be one of {sorted(FORMATS)}")
        self.k, self.m, self.x, self.use_ht = k, m, x, bool(use_ht)
        self.n_ranks, self.rank = n_ranks, rank
        self._cfg = make_config(k, m, x, B, use_ht, sequence_type, False, n_ranks, rank, device)
        self._device = device
        h = ctypes.c_void_p()
        _check(L.fk_create(ctypes.byref(self._cfg), ctypes.byref(h)))
        self._h = h
        self.num_bins = L.fk_num_bins(h)
        self.record_bytes = L.fk_record_bytes(h)
        self._keep = None
        self._sizes = None
        if (input_format, min_quality, quality_offset) != ("fasta", 0, 33):
            try:
                self.set_input_format(input_format, min_quality, quality_offset)
            except Exception:
                self.close()
                raise

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().fk_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- input
    def set_input_format(self, input_format: str = "fasta", min_quality: int = 0, quality_offset: int = 33) -> None:
        """The format of the next jobs' input (fk_set_input_format; between jobs only): "fasta", or
        "fastq" with bases of Phred score below min_quality counted as N (0: qualities ignored) under
        quality_offset 33 or 64."""
        if input_format not in FORMATS:
            raise ValueError(f"input_format must be one of {sorted(FORMATS)}")
        _check(lib().fk_set_input_format(self._h, FORMATS[input_format], int(min_quality), int(quality_offset)))

    def input_format(self) -> tuple:
        """(input_format, min_quality, quality_offset) as set."""
        f, q, o = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        _check(lib().fk_input_format(self._h, ctypes.byref(f), ctypes.byref(q), ctypes.byref(o)))
        return {v: n for n, v in FORMATS.items()}[f.value], q.value, o.value

    def fastq_info(self) -> dict:
        """After map() / finish() of a FASTQ job (also a failed one): its records, the bases masked by
        min_quality, and the index of the first malformed record (None: none)."""
        out = (ctypes.c_uint64 * 3)()
        _check(lib().fk_fastq_info(self._h, out))
        bad = int(out[2])
        return {"records": int(out[0]), "masked_bases": int(out[1]),
                "first_malformed": None if bad == 0xFFFFFFFFFFFFFFFF else bad}

    def fastq_stage_ms(self) -> tuple:
        """Measurement hook (fk_debug_fastq_ms): (device ms summed over the last FASTQ job's normalise
        launches, their number)."""
        ms, n = ctypes.c_double(), ctypes.c_uint64()
        _check(lib().fk_debug_fastq_ms(self._h, ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    def ingest(self, fasta: bytes) -> None:
        self._keep = bytes(fasta)
        _check(lib().fk_ingest(self._h, self._keep, len(self._keep), 1))

    def ingest_ptr(self, ptr: int, n: int, last: bool = True) -> None:
        """Append n host bytes at ptr (pinned memory is copied by DMA directly)."""
        _check(lib().fk_ingest(self._h, ctypes.cast(ptr, ctypes.c_char_p), n, 1 if last else 0))

    def ingest_chunk(self, chunk: bytes, last: bool) -> None:
        """Streamed input: append one chunk (the map of the landed bytes overlaps the copies)."""
        _check(lib().fk_ingest(self._h, chunk, len(chunk), 1 if last else 0))

    def reserve(self, total_bytes: int) -> None:
        """Size the device input for a streamed ingest of about total_bytes."""
        _check(lib().fk_ingest_reserve(self._h, total_bytes))

    def ingest_file_range(self, path: str, world: int | None = None, rank: int | None = None,
                          window_bytes: int = 0) -> None:
        """The job's input from a file: this rank's split (fk_ingest_file_range; world / rank
        default to the context's), read in pinned windows while earlier ones are copied and mapped."""
        _check(lib().fk_ingest_file_range(self._h, os.fsencode(path), self.n_ranks if world is None else world,
                                          self.rank if rank is None else rank, window_bytes))

    def balance_bins(self, sample: bytes) -> np.ndarray:
        """Size-aware placement (useCustomPartitioner) for the library's exchange, collective: the
        ranks' samples mapped, their per-bin k-mers summed, LPT owners installed; returns them."""
        _check(lib().fk_balance_bins(self._h, sample, len(sample)))
        return self.bin_owners()

    def balance_bins_file(self, path: str, fraction: float = 0.01, world: int | None = None,
                          rank: int | None = None) -> np.ndarray:
        """balance_bins from `fraction` of this rank's split of the file (the reference samples 1 %)."""
        _check(lib().fk_balance_bins_file(self._h, os.fsencode(path), self.n_ranks if world is None else world,
                                          self.rank if rank is None else rank, fraction))
        return self.bin_owners()

    def comm_allreduce(self, v) -> np.ndarray:
        """Collective: v summed over the job's ranks."""
        a = np.ascontiguousarray(v, dtype=np.uint64).copy()
        _check(lib().fk_comm_allreduce_u64(self._h, a.ctypes.data, a.size))
        return a

    def ingest_device(self, ptr: int, n: int) -> None:
        _check(lib().fk_ingest_device(self._h, ctypes.c_void_p(ptr), n, 1))

    def synth_device(self, n_reads: int, read_len: int = 100, genome_len: int = 100_000_000, seed: int = 0x5EED,
                     err_rate: float = 0.002, n_rate: float = 0.0005, first_read: int = 0) -> int:
        _check(lib().fk_synth_fasta_device(self._h, first_read, n_reads, read_len, genome_len, seed, err_rate,
                                           n_rate))
        return n_reads * lib().fk_synth_record_bytes(read_len)

    def set_stream(self, stream_ptr: int) -> None:
        _check(lib().fk_set_stream(self._h, ctypes.c_void_p(stream_ptr)))

    # -- map / shuffle / reduce
    def map(self) -> list[int]:
        self._sizes = None
        counts = (ctypes.c_uint64 * self.n_ranks)()
        _check(lib().fk_map(self._h, counts))
        return list(counts)

    def map_bin_kmers(self) -> np.ndarray:
        """After map(): k-mers per bin (all b bins) of this rank's records."""
        out = np.zeros(self.num_bins, dtype=np.uint64)
        _check(lib().fk_map_bin_kmers(self._h, out.ctypes.data))
        return out

    def bin_owners(self) -> np.ndarray:
        """The placement: owner rank of every bin."""
        out = np.zeros(self.num_bins, dtype=np.int32)
        _check(lib().fk_bin_owners(self._h, out.ctypes.data))
        return out

    def set_bin_owners(self, owner) -> list[int]:
        """Install a bin -> rank placement (identical on every rank); returns the
        send counts of the mapped records under it."""
        own = np.ascontiguousarray(owner, dtype=np.int32)
        if own.shape != (self.num_bins,):
            raise ValueError(f"owner table needs {self.num_bins} entries")
        counts = (ctypes.c_uint64 * self.n_ranks)()
        _check(lib().fk_set_bin_owners(self._h, own.ctypes.data, counts))
        self._sizes = None
        return list(counts)

    def map_emit(self, dst_ptr: int, cap_records: int) -> None:
        _check(lib().fk_map_emit(self._h, ctypes.c_void_p(dst_ptr), cap_records))

    def reduce(self, src_ptr: int, n_records: int) -> None:
        self._sizes = None
        _check(lib().fk_reduce(self._h, ctypes.c_void_p(src_ptr), n_records))

    def set_grouped_emit(self, enable: bool = True) -> int:
        """Group the emitted records by (destination, local bin); returns the
        parts per destination (fk_set_grouped_emit)."""
        _check(lib().fk_set_grouped_emit(self._h, 1 if enable else 0))
        return lib().fk_grouped_parts_per_rank(self._h)

    def map_part_counts(self):
        """After map() with grouped emit: (records, k-mers) per part, shape [n_ranks, parts]."""
        parts = lib().fk_grouped_parts_per_rank(self._h)
        rec = np.zeros(self.n_ranks * parts, dtype=np.uint64)
        km = np.zeros(self.n_ranks * parts, dtype=np.uint64)
        _check(lib().fk_map_part_counts(self._h, rec.ctypes.data, km.ctypes.data))
        return rec.reshape(self.n_ranks, parts), km.reshape(self.n_ranks, parts)

    def reduce_grouped(self, src_ptr: int, n_records: int, seg_records, seg_kmers) -> None:
        """Count records grouped by sender and local bin (fk_reduce_grouped);
        seg_records / seg_kmers: [n_senders, parts] arrays."""
        self._sizes = None
        sr = np.ascontiguousarray(seg_records, dtype=np.uint64)
        sk = np.ascontiguousarray(seg_kmers, dtype=np.uint64)
        if sr.shape != sk.shape or sr.ndim != 2:
            raise ValueError("seg_records and seg_kmers must be [n_senders, parts] arrays of one shape")
        _check(lib().fk_reduce_grouped(self._h, ctypes.c_void_p(src_ptr), n_records, sr.ctypes.data, sk.ctypes.data,
                                       sr.shape[0], sr.shape[1]))

    def finish(self) -> None:
        """Single rank: map + count.  With a communicator (comm_init / comm_init_local):
        the last piece, the exchange with the other ranks, and the count of this rank's
        bins -- collective, every rank of the job calls it."""
        self._sizes = None
        _check(lib().fk_finish(self._h))

    # -- multi-GPU inside the library (fk_comm_*)
    def comm_init(self, unique_id: bytes) -> None:
        """Join the job's RCCL communicator (unique_id from comm_unique_id() on one rank)."""
        if len(unique_id) != COMM_ID_BYTES:
            raise ValueError(f"an RCCL unique id has {COMM_ID_BYTES} bytes")
        buf = ctypes.create_string_buffer(bytes(unique_id), COMM_ID_BYTES)
        _check(lib().fk_comm_init(self._h, buf))

    @property
    def comm_transport(self) -> str:
        return lib().fk_comm_transport(self._h).decode()

    # -- results
    # min_count / max_count (results): only the k-mers with min_count <= count <= max_count, both ends
    # inclusive (max_count None: no upper bound), filtered on the device (fk_*_range); the defaults
    # are the unfiltered calls.
    def bin_sizes(self, min_count: int = 1, max_count: int | None = None) -> np.ndarray:
        out = np.zeros(self.num_bins, dtype=np.uint64)
        rg = _count_range(min_count, max_count)
        if rg is None:
            _check(lib().fk_bin_sizes(self._h, out.ctypes.data))
        else:
            _check(lib().fk_bin_sizes_range(self._h, rg[0], rg[1], out.ctypes.data))
        return out

    def get_bin(self, b: int, min_count: int = 1, max_count: int | None = None):
        n = ctypes.c_size_t(0)
        rg = _count_range(min_count, max_count)
        if self._sizes is None:
            self._sizes = self.bin_sizes()
        cnt = int(self._sizes[b])  # the unfiltered size bounds a filtered bin
        kw = 2 if self.k > 32 else 1
        keys = np.zeros(max(cnt, 1) * kw, dtype=np.uint64)
        counts = np.zeros(max(cnt, 1), dtype=np.uint32)
        if rg is None:
            _check(lib().fk_get_bin(self._h, b, keys.ctypes.data, counts.ctypes.data, max(cnt, 1), ctypes.byref(n)))
        else:
            _check(lib().fk_get_bin_range(self._h, b, rg[0], rg[1], keys.ctypes.data, counts.ctypes.data,
                                          max(cnt, 1), ctypes.byref(n)))
        return keys[:n.value * kw], counts[:n.value]

    # -- abundance spectrum (fk_spectrum*)
    def spectrum(self, n: int = 256, return_tail: bool = False):
        """The abundance spectrum of this rank's k-mers: a uint64 array of n >= 2 entries, hist[c] =
        distinct k-mers with count c for 1 <= c <= n - 2, hist[n - 1] = those with count >= n - 1
        (hist[0] = 0).  With return_tail also the sum of the counts of the k-mers in the last entry.
        The job's spectrum is the sum over the ranks (comm_allreduce)."""
        hist = np.zeros(max(int(n), 1), dtype=np.uint64)
        tail = ctypes.c_uint64(0)
        _check(lib().fk_spectrum(self._h, hist.ctypes.data, int(n), ctypes.byref(tail)))
        return (hist, int(tail.value)) if return_tail else hist

    def spectrum_ptr(self, d_hist: int, n: int, d_tail: int = 0) -> None:
        """fk_spectrum_device: the spectrum into uint64[n] at device pointer d_hist (and the tail's
        k-mer sum into uint64[1] at d_tail, if given), overwritten, queued on the context's stream
        (set_stream); nothing is allocated or synchronised."""
        _check(lib().fk_spectrum_device(self._h, ctypes.c_void_p(d_hist), int(n),
                                        ctypes.c_void_p(d_tail) if d_tail else None))

    # -- two-sample comparison (fk_compare*, fk_*_joined): this counter is sample A (walked), `other`
    # sample B (looked up in); same k, m, B, ranks, rank, owners and device, use_ht = False on both
    def compare(self, other: "KmerCounter", rows: int = 256, cols: int = 256) -> np.ndarray:
        """The joint count matrix, uint64 of shape (rows, cols): M[a, b] = distinct k-mers with count a
        here and count b in other (0: absent); the last row / column collect the counts >= rows - 1 /
        cols - 1; M[0, 0] = 0.  The job's matrix is the sum over the ranks (comm_allreduce)."""
        m = np.zeros((max(int(rows), 1), max(int(cols), 1)), dtype=np.uint64)
        _check(lib().fk_compare(self._h, other._h, m.ctypes.data, int(rows), int(cols)))
        return m

    def compare_ptr(self, other: "KmerCounter", d_matrix: int, rows: int, cols: int) -> None:
        """fk_compare_device: the matrix into uint64[rows * cols] at device pointer d_matrix,
        overwritten, queued on this counter's stream (set_stream) behind everything queued on other's;
        nothing is allocated or synchronised."""
        _check(lib().fk_compare_device(self._h, other._h, ctypes.c_void_p(d_matrix), int(rows), int(cols)))

    @staticmethod
    def _join_range(min_count, max_count, other_min, other_max):
        hi = MAX_COUNT if max_count is None else int(max_count)
        ohi = MAX_COUNT if other_max is None else int(other_max)
        rg = (int(min_count), hi, int(other_min), ohi)
        if not all(0 <= v <= MAX_COUNT for v in rg):
            raise ValueError("the counts of a joined range are 32-bit")
        return rg

    def bin_sizes_joined(self, other: "KmerCounter", min_count: int = 1, max_count: int | None = None,
                         other_min: int = 0, other_max: int | None = None) -> np.ndarray:
        """Per bin, this counter's k-mers with min_count <= count <= max_count whose count in other
        lies in [other_min, other_max] (0: absent from other; None: no upper bound)."""
        out = np.zeros(self.num_bins, dtype=np.uint64)
        rg = self._join_range(min_count, max_count, other_min, other_max)
        _check(lib().fk_bin_sizes_joined(self._h, other._h, *rg, out.ctypes.data))
        return out

    def get_bin_joined(self, other: "KmerCounter", b: int, min_count: int = 1, max_count: int | None = None,
                       other_min: int = 0, other_max: int | None = None):
        """(keys, counts, other_counts) of bin b's kept k-mers, in get_bin's order and layout."""
        n = ctypes.c_size_t(0)
        rg = self._join_range(min_count, max_count, other_min, other_max)
        if self._sizes is None:
            self._sizes = self.bin_sizes()
        cap = max(int(self._sizes[b]), 1) if 0 <= b < self.num_bins else 1  # the unfiltered size bounds a joined bin
        kw = 2 if self.k > 32 else 1
        keys = np.zeros(cap * kw, dtype=np.uint64)
        counts = np.zeros(cap, dtype=np.uint32)
        others = np.zeros(cap, dtype=np.uint32)
        _check(lib().fk_get_bin_joined(self._h, other._h, b, *rg, keys.ctypes.data, counts.ctypes.data,
                                       others.ctypes.data, cap, ctypes.byref(n)))
        return keys[:n.value * kw], counts[:n.value], others[:n.value]

    def intersect_bin(self, other: "KmerCounter", b: int):
        """Bin b's k-mers that other holds too: (keys, counts, other_counts)."""
        return self.get_bin_joined(other, b, other_min=1)

    def subtract_bin(self, other: "KmerCounter", b: int):
        """Bin b's k-mers that other lacks: (keys, counts, other_counts), the last all 0."""
        return self.get_bin_joined(other, b, other_min=0, other_max=0)

    # -- lookups in the counted result (fk_query*)
    def query(self, kmers, return_bins: bool = False):
        """Counts of k-mers (a list of strings, or a uint64 array in get_bin's layout; either
        strand): a uint32 array, 0 for an absent k-mer or a bin another rank owns.  With
        return_bins also the int32 bin of every k-mer (-1 for a key that is no k-mer)."""
        kw = 2 if self.k > 32 else 1
        if isinstance(kmers, np.ndarray):
            keys = np.ascontiguousarray(kmers, dtype=np.uint64).reshape(-1)
        else:
            keys = encode_keys(list(kmers), self.k)
        if keys.size % kw:
            raise ValueError("keys for k > 32 are (hi, lo) pairs")
        n = keys.size // kw
        counts = np.zeros(n, dtype=np.uint32)
        bins = np.zeros(n, dtype=np.int32) if return_bins else None
        _check(lib().fk_query(self._h, keys.ctypes.data, n, counts.ctypes.data,
                              bins.ctypes.data if return_bins else None))
        return (counts, bins) if return_bins else counts

    def query_ptr(self, d_keys: int, n: int, d_counts: int, d_bins: int = 0) -> None:
        """fk_query_device: n keys at device pointer d_keys -> uint32 counts at d_counts (and int32
        bins at d_bins, if given), queued on the context's stream (set_stream); nothing is
        allocated or synchronised."""
        _check(lib().fk_query_device(self._h, ctypes.c_void_p(d_keys), n, ctypes.c_void_p(d_counts),
                                     ctypes.c_void_p(d_bins) if d_bins else None))

    def query_sequence(self, seq) -> np.ndarray:
        """The count of every window seq[i, i + k) of a base sequence (str or bytes, no FASTA): a
        uint32 array of len(seq) - k + 1 entries (empty when shorter), 0 for a window holding a byte
        other than A/C/G/T."""
        raw = seq.encode() if isinstance(seq, str) else bytes(seq)
        n = ctypes.c_size_t(0)
        nwin = max(len(raw) - self.k + 1, 0)
        counts = np.zeros(nwin, dtype=np.uint32)
        _check(lib().fk_query_sequence(self._h, raw, len(raw), counts.ctypes.data if nwin else None, nwin,
                                       ctypes.byref(n)))
        return counts[:n.value]

    # -- per-read abundance profiles (fk_read_counts*, fk_read_stats*)
    def read_counts(self, bases, offsets, return_valid: bool = False):
        """The count of every window bases[p, p + k) of a CSR read batch (reads_csr), indexed by base
        position: a uint32 array of n_bases entries, 0 where no valid window starts (it would cross a read
        end or hold a byte other than A/C/G/T), for an absent k-mer or a bin another rank owns.  With
        return_valid also the uint8 array that is 1 exactly at the valid windows."""
        b, o = _csr_arrays(bases, offsets)
        counts = np.zeros(b.size, dtype=np.uint32)
        valid = np.zeros(b.size, dtype=np.uint8) if return_valid else None
        _check(lib().fk_read_counts(self._h, b.ctypes.data, o.ctypes.data, o.size - 1, counts.ctypes.data,
                                    valid.ctypes.data if return_valid else None))
        return (counts, valid) if return_valid else counts

    def read_stats(self, bases_or_text, offsets=None, min_count: int = 1, max_count: int | None = None,
                   input_format: str = "fasta", min_quality: int = 0, quality_offset: int = 33) -> np.ndarray:
        """Per-read statistics (a structured array mirroring fk_read_stat: windows, hits, min, median, max,
        reserved, sum) of a CSR batch (bases, offsets), or with offsets None of FASTA / FASTQ text cut by
        reads_csr.  hits counts the valid windows with min_count <= count <= max_count."""
        if offsets is None:
            bases_or_text, offsets = reads_csr(bases_or_text, input_format, min_quality, quality_offset)
        b, o = _csr_arrays(bases_or_text, offsets)
        hi = MAX_COUNT if max_count is None else int(max_count)
        if not (0 <= int(min_count) <= MAX_COUNT and 0 <= hi <= MAX_COUNT):
            raise ValueError("min_count / max_count are 32-bit counts")
        stats = np.zeros(o.size - 1, dtype=READ_STAT_DTYPE)
        _check(lib().fk_read_stats(self._h, b.ctypes.data, o.ctypes.data, o.size - 1, int(min_count), hi,
                                   stats.ctypes.data))
        return stats

    def read_counts_ptr(self, d_bases: int, d_offsets: int, n_reads: int, d_counts: int, d_valid: int = 0) -> None:
        """fk_read_counts_device: device pointers (uint8 bases, uint64 offsets[n_reads + 1], uint32
        counts[n_bases], uint8 valid[n_bases] if given), queued on the context's stream (set_stream);
        nothing is allocated or synchronised."""
        _check(lib().fk_read_counts_device(self._h, ctypes.c_void_p(d_bases), ctypes.c_void_p(d_offsets), n_reads,
                                           ctypes.c_void_p(d_counts), ctypes.c_void_p(d_valid) if d_valid else None))

    def read_stats_ptr(self, d_bases: int, d_offsets: int, n_reads: int, d_scratch: int, scratch_bytes: int,
                       d_stats: int, min_count: int = 1, max_count: int | None = None) -> None:
        """fk_read_stats_device: the window counts then the per-read reduction through the caller's
        scratch (read_stats_scratch_bytes(n_bases) bytes) into fk_read_stat[n_reads] at d_stats."""
        _check(lib().fk_read_stats_device(self._h, ctypes.c_void_p(d_bases), ctypes.c_void_p(d_offsets), n_reads,
                                          int(min_count), MAX_COUNT if max_count is None else int(max_count),
                                          ctypes.c_void_p(d_scratch), scratch_bytes, ctypes.c_void_p(d_stats)))

    def read_stats_of_counts_ptr(self, d_counts: int, d_valid: int, d_offsets: int, n_reads: int, d_stats: int,
                                 min_count: int = 1, max_count: int | None = None) -> None:
        """fk_read_stats_of_counts_device: per-read statistics of position-indexed device arrays (one
        rank's counts, or the ranks' summed); d_valid 0: every existing window is valid."""
        _check(lib().fk_read_stats_of_counts_device(self._h, ctypes.c_void_p(d_counts),
                                                    ctypes.c_void_p(d_valid) if d_valid else None,
                                                    ctypes.c_void_p(d_offsets), n_reads, int(min_count),
                                                    MAX_COUNT if max_count is None else int(max_count),
                                                    ctypes.c_void_p(d_stats)))

    # -- export, import and the database file (fk_export*, fk_import*, fk_save, fk_load); use_ht = False only
    def export_arrays(self):
        """The whole result as (keys, counts, bin_sizes): the bins this rank owns in the order of its
        local bins (ascending bin id under the default placement), each bin get_bin's keys and counts;
        bin_sizes (all num_bins entries) gives the cut points."""
        sizes = self.bin_sizes()
        d = int(sizes.sum())
        kw = 2 if self.k > 32 else 1
        keys = np.zeros(max(d, 1) * kw, dtype=np.uint64)
        counts = np.zeros(max(d, 1), dtype=np.uint32)
        n = ctypes.c_size_t(0)
        _check(lib().fk_export(self._h, keys.ctypes.data, counts.ctypes.data, max(d, 1), ctypes.byref(n)))
        return keys[:n.value * kw], counts[:n.value], sizes

    def export_ptr(self, d_keys: int, d_counts: int, cap: int) -> int:
        """fk_export_device: the same arrays at device pointers holding cap k-mers, queued on the context's
        stream (set_stream); returns the result's distinct k-mers."""
        n = ctypes.c_size_t(0)
        _check(lib().fk_export_device(self._h, ctypes.c_void_p(d_keys) if d_keys else None,
                                      ctypes.c_void_p(d_counts) if d_counts else None, int(cap), ctypes.byref(n)))
        return n.value

    def _bin_sizes_arg(self, bin_sizes) -> np.ndarray:
        sz = np.ascontiguousarray(bin_sizes, dtype=np.uint64).reshape(-1)
        if sz.size != self.num_bins:
            raise ValueError(f"bin_sizes needs {self.num_bins} entries")
        return sz

    def import_arrays(self, keys, counts, bin_sizes) -> None:
        """fk_import, the inverse of export_arrays: afterwards the counter is as after finish().
        FastKmerError (FK_E_INVALID) naming the bin, the index inside it and the reason for the first key
        that is no canonical k-mer of its bin in ascending order with a count >= 1."""
        kw = 2 if self.k > 32 else 1
        sz = self._bin_sizes_arg(bin_sizes)
        k = np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1)
        c = np.ascontiguousarray(counts, dtype=np.uint32).reshape(-1)
        if k.size != int(sz.sum()) * kw or c.size != int(sz.sum()):
            raise ValueError("keys and counts hold sum(bin_sizes) k-mers")
        self._sizes = None
        _check(lib().fk_import(self._h, k.ctypes.data, c.ctypes.data, sz.ctypes.data))

    def import_ptr(self, d_keys: int, d_counts: int, bin_sizes) -> None:
        """fk_import_device: keys and counts at device pointers, bin_sizes on the host."""
        sz = self._bin_sizes_arg(bin_sizes)
        self._sizes = None
        _check(lib().fk_import_device(self._h, ctypes.c_void_p(d_keys) if d_keys else None,
                                      ctypes.c_void_p(d_counts) if d_counts else None, sz.ctypes.data))

    def import_bins(self, bins: dict) -> None:
        """import_arrays from {bin: (keys, counts)}; bins left out are empty (default placement only)."""
        kw = 2 if self.k > 32 else 1
        sz = np.zeros(self.num_bins, dtype=np.uint64)
        ks, cs = [], []
        for b in sorted(bins):  # the local bins' order under the default placement
            k = np.ascontiguousarray(bins[b][0], dtype=np.uint64).reshape(-1)
            c = np.ascontiguousarray(bins[b][1], dtype=np.uint32).reshape(-1)
            if not 0 <= b < self.num_bins or k.size != c.size * kw:
                raise ValueError(f"bin {b}: outside [0, {self.num_bins}) or keys and counts of different lengths")
            sz[b] = c.size
            ks.append(k)
            cs.append(c)
        self.import_arrays(np.concatenate(ks) if ks else np.zeros(0, np.uint64),
                           np.concatenate(cs) if cs else np.zeros(0, np.uint32), sz)

    def save(self, path: str) -> None:
        """fk_save: the result as a database file (format: INTEGRATION.md "Saving and loading results")."""
        _check(lib().fk_save(self._h, os.fsencode(path)))

    def load_into(self, path: str) -> None:
        """fk_load into this counter: its k, m, bin count and key width must be the file's, and it must
        own every bin the file stores."""
        self._sizes = None
        _check(lib().fk_load(self._h, os.fsencode(path)))

    @classmethod
    def load(cls, path: str, x: int = 3, device: int = -1, n_ranks: int | None = None, rank: int | None = None):
        """A counter created from the file's header (k, m, bins) and loaded.  The file of one rank of a
        multi-rank job loads into a one-rank counter unless n_ranks / rank name the saver's."""
        h = db_info(path)
        kc = cls(h["k"], h["m"], x, h["bins"], n_ranks=1 if n_ranks is None else n_ranks,
                 rank=0 if rank is None else rank, device=device)
        try:
            kc.load_into(path)
        except Exception:
            kc.close()
            raise
        return kc

    def store_ms(self) -> dict:
        """Measurement hook (fk_debug_store_ms): the last save / load / import of this counter in ms."""
        out = (ctypes.c_double * 8)()
        _check(lib().fk_debug_store_ms(self._h, out))
        return {"wall": out[0], "device_copy": out[1], "host_copy_or_read": out[2], "write": out[3],
                "verify": out[4], "cells": out[5], "buckets": out[6]}

    def bin_dict(self, b: int, min_count: int = 1, max_count: int | None = None) -> dict:
        keys, counts = self.get_bin(b, min_count, max_count)
        return dict(zip(decode_keys(keys, self.k), (int(c) for c in counts)))

    def all_dict(self) -> dict:
        sizes = self.bin_sizes()
        return {b: self.bin_dict(b) for b in np.nonzero(sizes)[0].tolist()}

    def bin_text(self, b: int, min_count: int = 1, max_count: int | None = None) -> str:
        keys, counts = self.get_bin(b, min_count, max_count)
        lines = [f"{s}\t{int(c)}\n" for s, c in zip(decode_keys(keys, self.k), counts)]
        if not lines and _count_range(min_count, max_count) is not None:
            return ""  # a bin with no kept line has no file, so no trailer either
        return "".join(lines) + ("" if self.use_ht else "EOF")

    def write_bins(self, out_dir: str, min_count: int = 1, max_count: int | None = None) -> None:
        rg = _count_range(min_count, max_count)
        if rg is None:
            _check(lib().fk_write_bins(self._h, out_dir.encode()))
        else:
            _check(lib().fk_write_bins_range(self._h, out_dir.encode(), rg[0], rg[1]))

    # -- bin-signature diagnostics (executeFindBinSignaturesJob, SBKC:956-986)
    def signature_counts(self, out=None):
        """getBinSignatures (SBKC:772-917) over the ingested input: a device
        int64 tensor of 4^m + 1 super-k-mer counts indexed by signature value
        (``out``, if given, must hold that many).  The input stays ingested."""
        import torch
        n = lib().fk_signature_slots(self._h)
        if out is None:
            out = torch.empty(n, dtype=torch.int64, device=self._torch_device())
        if out.numel() < n or out.dtype != torch.int64 or not out.is_cuda or not out.is_contiguous():
            raise ValueError(f"signature counts need a contiguous device int64 tensor of {n} entries")
        _check(lib().fk_signature_counts(self._h, ctypes.c_void_p(out.data_ptr()), out.numel()))
        return out

    def write_bin_signatures(self, counts, out_dir: str) -> None:
        """saveBinSignatures (SBKC:920-953) for the bins this rank owns."""
        _check(lib().fk_write_bin_signatures(self._h, ctypes.c_void_p(counts.data_ptr()), counts.numel(),
                                             out_dir.encode()))

    def _torch_device(self):
        import torch
        return torch.device("cuda", self._device if self._device >= 0 else torch.cuda.current_device())

    def stats(self) -> dict:
        st = fk_stats()
        _check(lib().fk_get_stats(self._h, ctypes.byref(st)))
        return {n: getattr(st, n) for n, _ in fk_stats._fields_}

    def fold_stats(self) -> dict:
        """Test hook (fk_debug_fold_stats): the fold of the last finish()'s landed pieces -- pieces
        folded, their k-mers, the weighted entries they became, and the first piece's sampled
        entries per k-mer (None: no sample was taken)."""
        out = (ctypes.c_uint64 * 4)()
        _check(lib().fk_debug_fold_stats(self._h, out))
        return {"pieces_folded": int(out[0]), "entries_in": int(out[1]), "entries_out": int(out[2]),
                "sample_ratio": int(out[3]) / 1e6 if out[3] else None}

    def debug_count_pieces(self, F: int, keys, cell_counts, weighted: bool = False, fold_mask: int = 0) -> None:
        """Test hook (fk_debug_count_pieces): the staged count over the caller's pieces.  keys[p]:
        piece p's keys by (bin, cell) (uint64; (hi, lo) rows for k > 32), cell_counts[p]: its keys per
        cell (num_bins << F).  weighted: keys hold weight - 1 in bits [2k, 2k + 4); fold_mask: the
        pieces folded first.  Afterwards the counter is as after finish()."""
        kw = 1 if self.k <= 32 else 2
        ks = [np.ascontiguousarray(a, dtype=np.uint64).reshape(-1) for a in keys]
        cs = [np.ascontiguousarray(a, dtype=np.uint64).reshape(-1) for a in cell_counts]
        if len(ks) != len(cs):
            raise ValueError("one cell_counts array per piece")
        for a, n in zip(ks, cs):
            if n.size != self.num_bins << F or a.size != int(n.sum()) * kw:
                raise ValueError("a piece holds sum(cell_counts) keys in num_bins << F cells")
        ka = (ctypes.c_void_p * max(len(ks), 1))(*[a.ctypes.data for a in ks])
        ca = (ctypes.c_void_p * max(len(cs), 1))(*[a.ctypes.data for a in cs])
        self._sizes = None
        _check(lib().fk_debug_count_pieces(self._h, F, len(ks), ka, ca, int(bool(weighted)), fold_mask))

    def debug_tier_stats(self) -> dict:
        """Test hook (fk_debug_tier_stats): the last tiered count's census -- mid-tier buckets handed
        on to the 1024-key kernel, the split's fallbacks of at most / above 2048 keys, the buckets on
        the streaming path, and the mid tier's first kernel (None, "ranges" or "whole")."""
        out = (ctypes.c_uint64 * 8)()
        _check(lib().fk_debug_tier_stats(self._h, out))
        return {"nmidfb": int(out[0]), "nfbB": int(out[1]), "nfbG": int(out[2]), "nlarge": int(out[3]),
                "mid_mode": (None, "ranges", "whole")[int(out[4])]}

    def debug_staged_piece(self, p: int):
        """Test hook (fk_debug_staged_piece): (keys, cell offsets) of staged piece p of the last
        counted job as the count read it (after its fold, if any); the offsets cover
        num_bins << stats()["fine_bits"] cells."""
        kw = 1 if self.k <= 32 else 2
        cb = np.zeros((self.num_bins << self.stats()["fine_bits"]) + 1, dtype=np.uint64)
        _check(lib().fk_debug_staged_piece(self._h, p, None, cb.ctypes.data))
        keys = np.zeros(max(int(cb[-1]), 1) * kw, dtype=np.uint64)
        _check(lib().fk_debug_staged_piece(self._h, p, keys.ctypes.data, cb.ctypes.data))
        keys = keys[:int(cb[-1]) * kw]
        return (keys if kw == 1 else keys.reshape(-1, 2)), cb


def debug_wave_count(keys: np.ndarray, k: int, F: int, c0: int, c1: int, slots: int, device: int = 0,
                     weighted: bool = False):
    """Test hook (fk_debug_wave_count): one bucket of keys (uint64; (hi, lo) rows
    for k > 32) through the wave-tier count kernel; returns (distinct keys, counts).
    weighted (fk_debug_wave_count_w): k <= 30 keys may hold weight - 1 in bits [2k, 2k + 4)."""
    kw = 1 if k <= 32 else 2
    keys = np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1, kw)
    n = len(keys)
    ok = np.zeros(n * kw, dtype=np.uint64)
    oc = np.zeros(n, dtype=np.uint32)
    nout = ctypes.c_uint32(0)
    fn = lib().fk_debug_wave_count_w if weighted else lib().fk_debug_wave_count
    _check(fn(device, k, F, c0, c1, slots, keys.ctypes.data, n, ok.ctypes.data, oc.ctypes.data, ctypes.byref(nout)))
    u = nout.value
    return (ok[:u] if kw == 1 else ok[:2 * u].reshape(-1, 2)), oc[:u]


def live_resources() -> tuple[int, int, int, int]:
    """Test hook (fk_debug_live_resources): the device allocations, pinned host allocations, events and
    streams the library's contexts and calls hold in this process right now."""
    out = (ctypes.c_uint64 * 4)()
    _check(lib().fk_debug_live_resources(out))
    return tuple(int(v) for v in out)


def comm_unique_id() -> bytes:
    """A fresh RCCL unique id (fk_comm_unique_id): made on one rank, handed to all."""
    buf = ctypes.create_string_buffer(COMM_ID_BYTES)
    _check(lib().fk_comm_unique_id(buf))
    return buf.raw


def comm_init_local(counters) -> None:
    """Join KmerCounters of this process (ranks 0..n-1) into one in-process group
    (fk_comm_init_local); drive each from its own thread."""
    arr = (ctypes.c_void_p * len(counters))(*[c._h.value for c in counters])
    _check(lib().fk_comm_init_local(arr, len(counters)))


def exchange_plan(sent, received, record_bytes: int):
    """fk_exchange_plan: one exchange step's send / receive byte blocks.
    sent / received: [n_ranks, 2 * parts + 1] u64 messages.  Returns
    (send_off, send_bytes, recv_off, recv_bytes, all_final)."""
    snd = np.ascontiguousarray(sent, dtype=np.uint64)
    rcv = np.ascontiguousarray(received, dtype=np.uint64)
    if snd.ndim != 2 or snd.shape != rcv.shape or snd.shape[1] % 2 != 1:
        raise ValueError("sent / received must be [n_ranks, 2 * parts + 1] arrays of one shape")
    n, parts = snd.shape[0], (snd.shape[1] - 1) // 2
    so, sb, ro, rb = (np.zeros(n, dtype=np.uint64) for _ in range(4))
    fin = ctypes.c_int32(0)
    _check(lib().fk_exchange_plan(n, parts, snd.ctypes.data, rcv.ctypes.data, record_bytes, so.ctypes.data,
                                  sb.ctypes.data, ro.ctypes.data, rb.ctypes.data, ctypes.byref(fin)))
    return so, sb, ro, rb, bool(fin.value)


def lpt_owners(sizes, n_ranks: int) -> np.ndarray:
    """MultiprocessorSchedulingPartitioner.solve (MultiprocessorSchedulingPartitioner.scala:35-69):
    bins largest first onto the least loaded rank; bins of size 0 stay at bin % n_ranks."""
    sz = np.ascontiguousarray(sizes, dtype=np.uint64)
    owner = np.zeros(len(sz), dtype=np.int32)
    _check(lib().fk_lpt_owners(sz.ctypes.data, len(sz), n_ranks, owner.ctypes.data))
    return owner


def execute_job(configuration: TestConfiguration, input_format: str = "fasta", min_quality: int = 0,
                quality_offset: int = 33) -> KmerCounter:
    """SparkBinKmerCounter.executeJob (SparkBinKmerCounter.scala:989-1046) on one GPU.

    Reads the dataset, counts, and writes ``configuration.outputDir/bin<b>``
    when ``configuration.write`` is set.  Returns the counter (results stay
    device resident until it is closed).  ``input_format="fastq"`` reads a FASTQ
    dataset (KmerCounter.set_input_format).
    """
    with open(configuration.dataset, "rb") as f:
        data = f.read()
    kc = KmerCounter(configuration.k, configuration.m, configuration.x, configuration.max_b,
                     configuration.useHT, configuration.sequenceType, input_format=input_format,
                     min_quality=min_quality, quality_offset=quality_offset)
    kc.ingest(data)
    kc.finish()
    if configuration.write:
        kc.write_bins(configuration.outputDir)
    return kc


def execute_find_bin_signatures_job(configuration: TestConfiguration):
    """SparkBinKmerCounter.executeFindBinSignaturesJob (SBKC:956-986) on one GPU:
    per-signature super-k-mer counts of the dataset, written as
    ``configuration.outputDir/bin_signatures<b>.txt``.  Returns the counts (a
    device int64 tensor indexed by signature value)."""
    with open(configuration.dataset, "rb") as f:
        data = f.read()
    with KmerCounter(configuration.k, configuration.m, configuration.x, configuration.max_b,
                     configuration.useHT, configuration.sequenceType) as kc:
        kc.ingest(data)
        counts = kc.signature_counts()
        kc.write_bin_signatures(counts, configuration.outputDir)
    return counts
