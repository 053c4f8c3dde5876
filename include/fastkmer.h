/*
 * fastkmer.h -- C-ABI of the MI355X-native exact k-mer counter.
 *
 * Drop-in boundary for the hot path of maruscia/fastkmer: the body of
 *   SparkBinKmerCounter.executeJob(spark, configuration)
 *     src/main/scala/skc/SparkBinKmerCounter.scala:989-1046
 * i.e. the map closure getSuperKmers / getSuperKmersWithBinSizes (:34-169,
 * :290-426), the signature->bin shuffle reduceByKey (:1035, :1042) and the
 * reduce closures extractKXmers / extractKXmersHT (:428-660, :664-739).
 * INTEGRATION.md shows the JNI binding a Scala maintainer would add and the
 * ctypes binding used by this repository's tests.
 *
 * Plain C types only.  Every call returns FK_OK (0) or a negative FK_E_*
 * code and never aborts; fk_last_error() returns a thread-local message.
 * A context is used by one host thread at a time.  All GPU work runs on the
 * context's HIP stream on the device selected by fk_config.device.
 */
#ifndef FASTKMER_H
#define FASTKMER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version policy: bumped whenever an exported signature, a struct layout
 * (fk_config, fk_stats) or an error code's meaning changes; callers compare
 * fk_abi_version() with the FK_ABI_VERSION they were built against.
 *   3: fk_stats lost four always-zero fields (ht_spilled, ht_rounds, ms_merge,
 *      ht_big_groups); FK_E_COMM; fk_debug_comm_hold / _release / _held;
 *      fk_debug_fingerprint_bits. */
#define FK_ABI_VERSION 3

#define FK_OK 0
#define FK_E_INVALID (-1) /* bad argument or configuration (reference: require / AIOOBE) */
#define FK_E_STATE (-2)   /* call out of order (e.g. fk_get_bin before fk_finish) */
#define FK_E_DEVICE (-3)  /* HIP runtime failure or no usable GPU */
#define FK_E_NOMEM (-4)   /* device or host allocation failed */
#define FK_E_IO (-5)      /* file system error while writing bins */
#define FK_E_RANGE (-6)   /* caller buffer too small / bin out of range */
#define FK_E_COMM (-7)    /* a collective of the job failed or timed out (FASTKMER_COMM_TIMEOUT_S); the
                             communicator is aborted, later collective calls fail fast (reference: a failed
                             task fails the Spark job, SBKC:1031-1043) */

/* Mirrors skc.test.testutil.TestConfiguration (test/package.scala:16-42). */
typedef struct fk_config {
    int32_t k;             /* k-mer length, 1..64 (reference: any; Kmer packs 31 nt/Long) */
    int32_t m;             /* signature length, 1..15 (m >= 16 breaks Int shifts, SBKC:50) */
    int32_t x;             /* (k,x)-mer factor; must be >= 1 when use_ht == 0 (SBKC:435) */
    int32_t B;             /* requested bins; the library uses b = min(4^m, B) (package.scala:32) */
    int32_t use_ht;        /* 0: sorted count (extractKXmers), 1: hash count (extractKXmersHT) */
    int32_t sequence_type; /* 0: FASTA short reads, 1: long sequence (FASTdoop long format) */
    int32_t write;         /* reference "write" flag; only consulted by the CLI */
    int32_t n_ranks;       /* >= 1: bins are owned round-robin, bin % n_ranks == rank */
    int32_t rank;          /* 0..n_ranks-1 */
    int32_t device;        /* HIP device ordinal, -1 = current device */
} fk_config;

typedef struct fk_ctx fk_ctx;

/* Per-context statistics (device times are HIP-event times on the ctx stream). */
typedef struct fk_stats {
    uint64_t fasta_bytes;      /* bytes ingested */
    uint64_t positions;        /* sequence positions after FASTA parsing */
    uint64_t bases;            /* A/C/G/T/N... sequence bytes (input bases) */
    uint64_t kmers;            /* valid k-mer windows counted */
    uint64_t superkmers;       /* super-k-mer records produced by fk_map */
    uint64_t records_received; /* records counted by fk_reduce */
    uint64_t distinct;         /* distinct canonical k-mers owned by this rank */
    uint64_t oversize_buckets; /* buckets that took the large-bucket path */
    uint64_t buckets;          /* LDS count buckets (sorted path) */
    uint64_t fine_bits;        /* cell bits F below the bin (sorted path) */
    double ms_parse;           /* FASTA parse + 2-bit encode kernels */
    double ms_signature;       /* signature / super-k-mer kernel */
    double ms_partition;       /* record partition kernels */
    double ms_count;           /* expand + bucket + sort/hash + compact kernels */
    double ms_total;           /* fk_map + fk_reduce wall time on the host */
    double ms_encode_kernel;   /* last launch of the encode kernel */
    double ms_signature_kernel;/* last launch of the signature kernel (the fused parse + signature kernel when fused_map) */
    uint64_t fused_map;        /* 1: the last fk_map ran the fused kernel (k_map_fused), 0: parse + signature kernels */
    double ms_h2d;             /* last fk_ingest: host-to-device copy, first segment issued to last landed */
    uint64_t fused_fallback;   /* why the fused kernel handed the input back: 1 long line, 2 text before the
                                  first header, 4 halo too short, 8 too many records in a tile (0: none) */
    /* multi-rank exchange inside the context (fk_comm_init*), last fk_finish */
    uint64_t xch_steps;        /* exchange steps (pieces sent during fk_ingest, the last piece, closing steps) */
    uint64_t xch_bytes_sent;   /* record bytes sent to other ranks */
    uint64_t xch_bytes_received; /* record bytes received from other ranks */
    double ms_exchange;        /* sum over the steps of their record transfer time on the comm stream */
    double ms_exchange_tail;   /* fk_finish: the last piece posted -> every rank's records received */
    /* pieces counted while later ones were still being copied in / received (sorted count) */
    uint64_t pieces_counted;   /* staged pieces of the last fk_finish (0: one count of the whole input) */
    uint64_t heavy_keys;       /* sorted count: k-mers in the buckets above the wave tier (split or block / big);
                                  with folded pieces (fk_debug_fold_stats) this and the buckets' sizes count
                                  staged entries, a folded entry standing for up to 15 occurrences */
    uint64_t block_buckets;    /* block tier: buckets above the wave tier (k <= 32: 512 keys, k > 32: 256) counted by
                                  the mid wave tier, one wave each: up to 1024 keys (k <= 32) / 512 keys (k > 32) */
    uint64_t big_buckets;      /* above the block tier: split into wave-sized sub-buckets (k_bucket_split64 /
                                  k_bucket_split128) counted in order by one wave per bucket (k_sub_count64_seq /
                                  k_sub_count128_seq); fallbacks only for a bucket the split cannot cut (a k-mer
                                  repeated too often): the block kernel (k <= 32) / LDS sort (k > 32) up to 2048
                                  keys, above it the big-table kernel (k <= 32) and the streaming path */
    uint64_t split_buckets;    /* big-tier buckets the split cut into wave-sized sub-buckets (not the fallbacks) */
    uint64_t sub_buckets;      /* ... into this many sub-buckets (one wave per bucket counted them in order) */
} fk_stats;

/* ---- host-only helpers (no GPU needed) ---------------------------------- */

int fk_abi_version(void);
/* Defaults of LocalTestKmerCounter.main (LocalTestKmerCounter.scala:20-33). */
int fk_config_init(fk_config *cfg);
/* Validates without touching the GPU; FK_E_INVALID with a message on error. */
int fk_config_validate(const fk_config *cfg);
/* b = min(4^m, B) exactly as TestConfiguration.b (test/package.scala:32). */
int32_t fk_clamped_bins(int32_t m, int32_t B);
/* TestConfiguration.outputDir (test/package.scala:33, debug == false). */
int fk_output_dir(const fk_config *cfg, const char *output_path, const char *prefix, char *out, size_t cap);
/* Bytes of one packed super-k-mer record for k (16 for k <= 32, 24 for k <= 64). */
size_t fk_record_bytes_for_k(int32_t k);
/* Deterministic synthetic short-read FASTA (">r%010d\n" + read + "\n"),
 * identical on host and device; see fk_synth_fasta_device. */
uint64_t fk_synth_record_bytes(int32_t read_len);
int fk_synth_fasta_host(uint8_t *out, uint64_t first_read, uint64_t n_reads, int32_t read_len,
                        uint64_t genome_len, uint64_t seed, double err_rate, double n_rate);

/* ---- context ------------------------------------------------------------ */

int fk_create(const fk_config *cfg, fk_ctx **out);
void fk_destroy(fk_ctx *ctx);
const char *fk_last_error(void);
/* Optional: run on a caller-owned hipStream_t (e.g. torch's current stream). */
int fk_set_stream(fk_ctx *ctx, void *hip_stream);

/* Input.  fk_ingest copies host FASTA bytes to the device (may be called
 * repeatedly: the chunks are concatenated; last = 1 marks the final chunk).
 * The copy runs in segments on the context's copy stream and, for the fused
 * map configurations, every tile whose bytes have landed is mapped while the
 * next segment is in flight; the call returns once the source has been read.
 * fk_ingest_device borrows a device buffer (zero-copy; it must stay valid
 * until fk_map returns, and one borrowed input is mapped once). */
int fk_ingest(fk_ctx *ctx, const uint8_t *fasta, size_t n, int last);
/* Optional, before a streamed fk_ingest sequence: size the device input for
 * about total_bytes, so the copies of later chunks overlap the map without a
 * reallocation (FASTdoop-style streaming ingest).  The size also
 * places the job's piece cuts and sizes its cells, as for a job passed in one
 * fk_ingest call (a wrong size costs time, never results). */
int fk_ingest_reserve(fk_ctx *ctx, uint64_t total_bytes);
int fk_ingest_device(fk_ctx *ctx, const void *d_fasta, size_t n, int last);
/* A rank's input split of a FASTA file, as the reference's FASTdoop input
 * formats cut it for its map tasks (SBKC:993, 1009-1012): the file is cut into
 * byte ranges of ~size/world.  sequence_type 0 (FASTAshortInputFileFormat):
 * the whole records whose '>' lies in the rank's range.  sequence_type 1
 * (FASTAlongInputFileFormat, overlap key "k"): the k-mer windows whose first
 * base lies in the range -- a header line ">s\n", the range's bytes (after a
 * header line it starts inside; nothing before the file's first header), the
 * k - 1 sequence positions after it (stopping at a record boundary), "\n".
 * The union of the ranks' counts is the whole file's.
 *   fk_split_bytes: host only; the bytes rank `rank` ingests into out (cap
 *     bytes; out = NULL: only *n, the split's size).
 *   fk_ingest_file_range: the whole job input of this context from the file
 *     (a fresh job, as one fk_ingest sequence with last = 1 at its end): the
 *     split of (k, sequence_type) of the context's configuration, read with
 *     positioned reads into two pinned windows of window_bytes (0: 256 MB;
 *     the next window is read while the last one is copied and mapped), the
 *     job's size announced first (fk_ingest_reserve).  Collective like
 *     fk_ingest with a communicator.  world / rank: the split (usually the
 *     context's n_ranks / rank; with a communicator they must be, else
 *     FK_E_INVALID). */
int fk_split_bytes(const char *path, int32_t world, int32_t rank, int32_t k, int32_t sequence_type, uint8_t *out,
                   size_t cap, size_t *n);
int fk_ingest_file_range(fk_ctx *ctx, const char *path, int32_t world, int32_t rank, uint64_t window_bytes);
/* ---- FASTQ input (the reference marks the gap: its FASTQInputFileFormat lines
 * are commented out, SBKC:975, 1007) ----
 * Strict four-line records: "@name", sequence, "+[anything]", quality; one line
 * each (no wrapped sequences), LF or CRLF, the final newline may be missing,
 * blank lines may trail the input, reads may be empty, quality lines may begin
 * with or contain '@', '+' or '>'.  Sequence bytes follow the FASTA rules: only
 * ACGT are valid; N, lowercase, IUPAC codes and '\r' are invalid positions.  A
 * record starts at a line beginning with '@' whose second-next line begins with
 * '+' (exact for this grammar).
 * A small device stage in front of the FASTA parse rewrites the device input in
 * place, at the same byte offsets: the '@', the '+' and the first byte of a
 * non-empty quality line become '>' (the '+' and quality lines are header lines
 * to the parser), and with min_quality > 0 every base whose Phred score
 * (quality byte - quality_offset) is below it becomes 'N'.  fk_stats.kmers,
 * distinct and every result call then equal those of the equivalent FASTA job
 * ('@' -> '>', the '+' and quality lines dropped, masked bases as 'N');
 * fk_stats.fasta_bytes is the FASTQ bytes ingested, and fk_stats.positions
 * counts the sequence bytes plus one separator per header line the parser sees:
 * three per record (two for a record with an empty quality line).
 * The format applies to fk_ingest (one call or chunks, pinned or pageable),
 * fk_ingest_device (the borrowed buffer is left as it is: the stage copies it
 * into the context's own input; less than 4 GiB per call), fk_ingest_file_range
 * (the FASTQ split), fk_balance_bins (a sample of whole FASTQ records),
 * fk_signature_counts and jobs with a communicator.  fk_balance_bins_file
 * returns FK_E_INVALID on a FASTQ context.
 * Malformed input -- a record without its '@' or its '+', a quality line whose
 * length differs from the sequence's, an input ending inside a record -- makes
 * the job's fk_map / fk_finish return FK_E_INVALID, the message naming the
 * first malformed record (0-based); the context takes a new job afterwards.
 * An input with more than one line per 4 bytes over a stretch of it (reads of
 * under 5 bases throughout) is refused the same way. */
#define FK_FORMAT_FASTA 0
#define FK_FORMAT_FASTQ 1
/* Between jobs only (FK_E_STATE after a job's first fk_ingest and before its
 * fk_finish / fk_map).  FASTQ needs sequence_type == 0 (else FK_E_INVALID).
 * min_quality: Phred score below which a base counts as N (0: qualities are
 * ignored; at most 93); quality_offset: 33 or 64.  (FASTA, 0, 33) is the
 * default and is exactly the FASTA-only behaviour, with no extra launch. */
int fk_set_input_format(fk_ctx *ctx, int32_t format, int32_t min_quality, int32_t quality_offset);
int fk_input_format(const fk_ctx *ctx, int32_t *format, int32_t *min_quality, int32_t *quality_offset);
/* After fk_finish / fk_map of a FASTQ job (also one that failed on a malformed
 * record): out[0] = records, out[1] = bases whose quality is below min_quality
 * (whatever the base), out[2] = index of the first malformed record
 * (UINT64_MAX: none).  FK_E_STATE before the first such job. */
int fk_fastq_info(fk_ctx *ctx, uint64_t out[3]);
/* Host only.  The offset of the start of the last record whose '@' line and
 * '+' line both begin inside buf[0, n): the last line start L with
 * buf[L] == '@' such that the line two after L exists and begins with '+'
 * (buf[0] counts as a line start).  *off = n when there is none.  A streamed
 * fk_ingest maps only below this frontier: the record it names may be
 * incomplete. */
int fk_fastq_frontier(const uint8_t *buf, size_t n, size_t *off);
/* Host only: fk_split_bytes for a FASTQ file (sequence_type 0 semantics: the
 * whole records whose '@' line starts in the rank's byte range; rank 0 also
 * gets what precedes the first record start). */
int fk_split_bytes_fastq(const char *path, int32_t world, int32_t rank, uint8_t *out, size_t cap, size_t *n);

/* Fill a caller's device buffer (current device) with the same bytes as
 * fk_synth_fasta_host (benchmarks: the input is staged to pinned host memory). */
int fk_synth_fasta_to_device(void *d_out, uint64_t first_read, uint64_t n_reads, int32_t read_len,
                             uint64_t genome_len, uint64_t seed, double err_rate, double n_rate);
/* Fill the device input with fk_synth_fasta-compatible data (benchmarks). */
int fk_synth_fasta_device(fk_ctx *ctx, uint64_t first_read, uint64_t n_reads, int32_t read_len,
                          uint64_t genome_len, uint64_t seed, double err_rate, double n_rate);

/* Map side (getSuperKmers, SBKC:34-169): parse, encode, signature,
 * super-k-mer records; send_counts[r] = records destined to rank r. */
int fk_map(fk_ctx *ctx, uint64_t *send_counts);
size_t fk_record_bytes(const fk_ctx *ctx);
/* Write the mapped records into d_send grouped by destination rank
 * (rank 0 first), send_counts as returned by fk_map. */
int fk_map_emit(fk_ctx *ctx, void *d_send, uint64_t cap_records);
/* Reduce side (reduceByKey + extractKXmers[HT]): count the records in
 * d_recv (device memory, fk_record_bytes each, all owned by this rank). */
int fk_reduce(fk_ctx *ctx, const void *d_recv, uint64_t n_records);
/* Grouped exchange (default placement only): with fk_set_grouped_emit(ctx, 1)
 * before fk_map, fk_map_emit groups the records by (destination rank, local
 * bin) -- the reduceByKey grouping of SBKC:1035 done on the sender -- and
 * fk_map_part_counts returns records / k-mers per part ([n_ranks][parts],
 * parts = fk_grouped_parts_per_rank).  A receiver then skips its partition
 * pass: fk_reduce_grouped counts d_recv = n_seg segments (one per sender, in
 * order), each holding seg_records[s * parts + lb] records of local bin lb,
 * bin after bin. */
int fk_set_grouped_emit(fk_ctx *ctx, int32_t enable);
int32_t fk_grouped_parts_per_rank(const fk_ctx *ctx);
int fk_map_part_counts(fk_ctx *ctx, uint64_t *records, uint64_t *kmers);
int fk_reduce_grouped(fk_ctx *ctx, const void *d_recv, uint64_t n_records, const uint64_t *seg_records,
                      const uint64_t *seg_kmers, int32_t n_seg, int32_t parts_per_seg);
/* Single rank: fk_map + fk_reduce on the local records. */
int fk_finish(fk_ctx *ctx);

/* Size-aware bin placement, the MultiprocessorSchedulingPartitioner of the
 * reference (SBKC:1023-1025, MultiprocessorSchedulingPartitioner.scala:35-69)
 * with exact sizes instead of a 1% sample.  Default placement: bin % n_ranks.
 *   fk_map_bin_kmers: after fk_map, the k-mers per bin of this rank's records
 *     (all b bins); sum them over the ranks (e.g. an all-reduce),
 *   fk_lpt_owners: largest bin first onto the least loaded rank (host only;
 *     bins of size 0 keep bin % n_ranks),
 *   fk_set_bin_owners: install owner[b] (the same table on every rank) before
 *     fk_map_emit / fk_reduce, or before a job's first fk_ingest with a
 *     communicator (the exchange then groups records by (owner, the bin's index
 *     among its owner's bins)); when already mapped it recomputes send_counts
 *     (and, with the grouped emit, fk_map_part_counts) under the new owners, so
 *     fk_map_emit may follow directly. */
int fk_map_bin_kmers(fk_ctx *ctx, uint64_t *kmers_per_bin);
int fk_lpt_owners(const uint64_t *sizes, int32_t nbins, int32_t nranks, int32_t *owner);
int fk_set_bin_owners(fk_ctx *ctx, const int32_t *owner, uint64_t *send_counts);
/* The context's placement: owner[b] for all b bins (bin % n_ranks unless set). */
int fk_bin_owners(const fk_ctx *ctx, int32_t *owner);

/* ---- multi-GPU inside the context (one context per GPU) --------
 * The job's contexts (fk_config.n_ranks = n, rank = 0..n-1) join one
 * communicator.  A context then exchanges its records itself: fk_ingest
 * groups every landed piece of its input (FASTKMER_PIECE_BYTES, 1 GB) by
 * (owner rank, local bin) and sends it while the next piece is still being
 * copied in; fk_finish sends the last piece, receives every rank's, and
 * counts the bins this rank owns (bin % n_ranks), as the executors of the
 * reference's reduceByKey shuffle do (SBKC:1034-1042).  fk_finish (and
 * fk_ingest, which may send pieces) are collective: every rank of the job
 * calls them, each from its own host thread or process.  Ranks may hold
 * different amounts of input: a rank that has sent its last piece keeps
 * answering the others' steps inside fk_finish.
 * Failure semantics (the reference fails the whole Spark job when one task
 * fails: require at package.scala:182,185, exceptions out of SBKC:1031-1043):
 * every host wait on RCCL work is bounded -- it polls the stream and
 * ncclCommGetAsyncError, and after FASTKMER_COMM_TIMEOUT_S seconds (default
 * 120) or an asynchronous RCCL error it aborts the communicator
 * (ncclCommAbort) and the call returns FK_E_COMM; any failing collective call
 * aborts it too, so the peers' waits end instead of blocking.
 * FASTKMER_COMM_SPLIT=0 keeps the per-step count exchange on the records'
 * communicator and stream (default: a communicator split off it, with its own
 * stream). */
#define FK_COMM_ID_BYTES 128
/* A fresh RCCL unique id (ncclGetUniqueId): made on one rank, handed to all. */
int fk_comm_unique_id(uint8_t id[FK_COMM_ID_BYTES]);
/* RCCL over xGMI: joins the job's communicator (blocks until every rank has joined). */
int fk_comm_init(fk_ctx *ctx, const uint8_t id[FK_COMM_ID_BYTES]);
/* n contexts of this process as ranks 0..n-1 (created with n_ranks = n): records move
 * by device-to-device copies; drive each context from its own host thread. */
int fk_comm_init_local(fk_ctx **ctxs, int32_t n);
/* "rccl", "local" or "" (no communicator). */
const char *fk_comm_transport(const fk_ctx *ctx);
/* Collective: v[0..n) summed over the job's ranks (in place). */
int fk_comm_allreduce_u64(fk_ctx *ctx, uint64_t *v, size_t n);
/* Size-aware placement for the library's exchange (useCustomPartitioner:
 * SBKC:1023-1026, MultiprocessorSchedulingPartitioner.scala:35-69), collective,
 * before a job's first fk_ingest: every rank maps a sample of its input (never
 * exchanged), the per-bin k-mer totals are summed over the ranks, and the LPT
 * placement (fk_lpt_owners) is installed on every rank (fk_set_bin_owners);
 * the job's records then go to their bin's owner.  Without a communicator the
 * rank's own sample decides.
 *   fk_balance_bins: the caller's sample bytes (FASTA text);
 *   fk_balance_bins_file: `fraction` of the rank's split of the file (evenly
 *     spaced blocks; the reference samples 1 %); world / rank as for
 *     fk_ingest_file_range. */
int fk_balance_bins(fk_ctx *ctx, const uint8_t *sample, size_t n);
int fk_balance_bins_file(fk_ctx *ctx, const char *path, int32_t world, int32_t rank, double fraction);
/* Host-only arithmetic of one exchange step.  sent[d * (2 * parts + 1) + i] is this
 * rank's message to rank d: records of local bin i (i < parts), k-mers of local bin
 * i - parts, then a flag word (bit 0: the sender's last piece, bit 1: the sender
 * retracts its earlier pieces); received[] holds every sender's message to this
 * rank in the same layout.  Fills the byte offsets and sizes of the step's send
 * blocks (records grouped by destination, rank 0 first) and receive blocks (by
 * sender), and *all_final (every sender has sent its last piece). */
int fk_exchange_plan(int32_t n_ranks, int32_t parts, const uint64_t *sent, const uint64_t *received,
                     uint64_t record_bytes, uint64_t *send_off, uint64_t *send_bytes, uint64_t *recv_off,
                     uint64_t *recv_bytes, int32_t *all_final);

/* ---- results (device resident; copied out on request) ------------------ */

int32_t fk_num_bins(const fk_ctx *ctx); /* b = min(4^m, B) */
/* distinct[b] for all b (0 for bins owned by other ranks). */
int fk_bin_sizes(fk_ctx *ctx, uint64_t *distinct_per_bin);
/* Canonical k-mers of bin b and their counts.  useHT=0: ascending
 * lexicographic order (extractKXmers); useHT=1: table order.  keys hold one
 * word per k-mer for k <= 32 and two (first k-32 bases, last 32 bases) for
 * k > 32, 2 bits per base, A=0 C=1 G=2 T=3, most significant base first. */
int fk_get_bin(fk_ctx *ctx, int32_t bin, uint64_t *keys, uint32_t *counts, size_t cap, size_t *n);
/* Reference byte format: <out_dir>/bin<b>, "<kmer>\t<count>\n" lines, plus
 * "EOF" (no newline) when use_ht == 0 (SBKC:550-606, :715-734). */
int fk_write_bins(fk_ctx *ctx, const char *out_dir);
int fk_get_stats(fk_ctx *ctx, fk_stats *out);

/* ---- lookups in the counted result (no reference counterpart) ----
 * How often does a k-mer occur?  Keys use fk_get_bin's layout (one word for
 * k <= 32, (hi, lo) for k > 32, 2 bits per base, most significant base first)
 * and may be on either strand: the library canonicalises them.
 *   counts[i]: occurrences of the canonical k-mer in the job's input when this
 *     rank owns the k-mer's bin, else 0; 0 for a k-mer the input does not hold.
 *   bins (may be NULL): bins[i] = the k-mer's bin in [0, b), whoever owns it.
 * A key with a bit set above bit 2k - 1 is no k-mer: count 0, bin -1.
 * The calls are not collective and move nothing between ranks: the sum of the
 * ranks' counts is the job's answer, and bins with fk_bin_owners lets a caller
 * route its queries.  They need a result (FK_E_STATE before fk_finish /
 * fk_reduce and after a new job's first fk_ingest) of the sorted count
 * (use_ht == 1: FK_E_INVALID, its results are in table order), read it only,
 * and answer the same before and after fk_get_bin / fk_write_bins.
 *   fk_query: host pointers; staged through the context's device buffers in
 *     chunks of FASTKMER_QUERY_CHUNK keys (default 16 Mi); returns once counts
 *     and bins are filled.
 *   fk_query_device: pointers on the context's device (d_counts uint32[n],
 *     d_bins int32[n] or NULL); only queues the lookup on the context's stream
 *     (the caller's after fk_set_stream): no allocation, no synchronisation.
 *   fk_query_sequence: seq holds bases only (no FASTA); *n = len - k + 1
 *     windows (0 when len < k), counts[i] = the count of seq[i, i + k), 0 for a
 *     window with a byte other than A/C/G/T (N, lowercase, newline).
 *     FK_E_RANGE when cap < *n; counts == NULL: only *n. */
/* Host only: the bin of a k-mer under cfg (k, m, B): hash_to_bucket(the minimum
 * norm over its k - m + 1 m-mers, b).  FK_E_INVALID for a configuration
 * fk_config_validate refuses or a key that is no k-mer. */
int fk_kmer_bin(const fk_config *cfg, const uint64_t *key, int32_t *bin);
int fk_query(fk_ctx *ctx, const uint64_t *keys, size_t n, uint32_t *counts, int32_t *bins);
int fk_query_device(fk_ctx *ctx, const void *d_keys, size_t n, void *d_counts, void *d_bins);
int fk_query_sequence(fk_ctx *ctx, const uint8_t *seq, size_t len, uint32_t *counts, size_t cap, size_t *n);

/* ---- abundance spectrum and count ranges (no reference counterpart) ----
 * What a k-mer count is used for first: the histogram "how many distinct
 * k-mers occur c times" (jellyfish histo, kmc_tools histogram), and output
 * with count cut-offs (-ci / -cx, -L / -U: drop the singletons, keep counts in
 * [lo, hi]).  Both are computed on the device from the counted result, for
 * use_ht == 0 and use_ht == 1 alike; the calls read the result only:
 * fk_get_bin, fk_write_bins and fk_query answer the same before and after
 * them.  They need a result (FK_E_STATE before fk_finish / fk_reduce and after
 * a new job's first fk_ingest); an empty job answers with zeros and writes no
 * files.  None of them is collective.
 *   fk_spectrum: hist has n >= 2 entries (else FK_E_INVALID).  hist[0] = 0;
 *     hist[c], 1 <= c <= n - 2: the distinct canonical k-mers this rank owns
 *     with count exactly c; hist[n - 1]: those with count >= n - 1, and
 *     *tail_kmers (may be NULL) the sum of their counts.  So the sum of hist is
 *     the rank's distinct k-mers (fk_stats.distinct), and the sum of
 *     c * hist[c] over c < n - 1 plus *tail_kmers its counted k-mer windows.
 *     The job's spectrum is the sum of the ranks': fk_comm_allreduce_u64 on
 *     hist (and on tail_kmers) gives it.
 *   fk_spectrum_device: pointers on the context's device (d_hist uint64[n],
 *     d_tail_kmers uint64[1] or NULL); only queues the work on the context's
 *     stream (the caller's after fk_set_stream): no allocation, no
 *     synchronisation.  The outputs are overwritten, not accumulated into.
 * Count ranges: a k-mer is kept when min_count <= count <= max_count, both
 * ends inclusive; max_count = UINT32_MAX: no upper bound.  FK_E_INVALID for
 * min_count == 0 or min_count > max_count.  (1, UINT32_MAX) gives exactly what
 * fk_bin_sizes / fk_get_bin / fk_write_bins give.
 *   fk_bin_sizes_range: kept k-mers per bin, all b bins (0 for bins owned by
 *     other ranks).
 *   fk_get_bin_range: fk_get_bin's order with the other k-mers removed
 *     (ascending for use_ht == 0, table order for use_ht == 1) and its buffer
 *     rules: *n is always set, FK_E_RANGE when cap < *n or the bin is out of
 *     [0, b); keys and counts may each be NULL.
 *   fk_write_bins_range: <out_dir>/bin<b> files of the kept lines only, "EOF"
 *     after the last kept line when use_ht == 0; a bin with no kept line gets
 *     no file, as an empty bin gets none from fk_write_bins. */
int fk_spectrum(fk_ctx *ctx, uint64_t *hist, size_t n, uint64_t *tail_kmers);
int fk_spectrum_device(fk_ctx *ctx, void *d_hist, size_t n, void *d_tail_kmers);
int fk_bin_sizes_range(fk_ctx *ctx, uint32_t min_count, uint32_t max_count, uint64_t *distinct_per_bin);
int fk_get_bin_range(fk_ctx *ctx, int32_t bin, uint32_t min_count, uint32_t max_count,
                     uint64_t *keys, uint32_t *counts, size_t cap, size_t *n);
int fk_write_bins_range(fk_ctx *ctx, const char *out_dir, uint32_t min_count, uint32_t max_count);

/* ---- two-sample comparison (no reference counterpart) ----
 * Two counted sets compared on the device: reads against an assembly (KAT
 * comp, the spectra-cn plot), sample against sample, a sample against a panel
 * (kmc_tools simple: intersect, kmers_subtract, counters_subtract).  ctx is
 * sample A, whose result is walked; other is sample B, in whose result every
 * k-mer of A is looked up.  ctx == other is allowed.
 * Compatibility: both contexts must have the same k, m, clamped bin count,
 * n_ranks and rank, equal fk_bin_owners tables, the same device and use_ht ==
 * 0 (a use_ht == 1 result cannot be looked up); x may differ.  Anything else
 * is FK_E_INVALID with a message naming the mismatch.  Both must hold a result
 * (else FK_E_STATE); an empty result on either side is fine and answers with
 * zeros, or with only row 0 / column 0 filled.
 * The calls read both results only: fk_get_bin, fk_write_bins, fk_query and
 * fk_spectrum on both contexts answer the same before and after them.  None is
 * collective: each rank answers for the bins it owns.
 * Streams: the work runs on ctx's stream (the caller's after fk_set_stream).
 * Before it is queued, ctx's stream is made to wait for an event recorded on
 * other's stream, so other's result is complete however the caller's streams
 * are arranged.  While a _device call is outstanding, other must not start a
 * new job (its first fk_ingest) and must not be destroyed.
 *   fk_compare: the joint count matrix, row-major uint64[rows][cols], overwritten
 *     (not accumulated into): matrix[a][b] = the distinct canonical k-mers with
 *     count a in ctx and count b in other, 0 meaning absent; the last row
 *     collects the counts >= rows - 1 of ctx, the last column the counts >=
 *     cols - 1 of other; matrix[0][0] = 0.  So row a >= 1 sums to fk_spectrum's
 *     entry a of ctx, column b >= 1 to that of other.  2 <= rows, cols <= 65536
 *     and rows * cols <= 2^24, else FK_E_INVALID.  The job's matrix is the sum
 *     of the ranks': fk_comm_allreduce_u64 on the matrix gives it.
 *   fk_compare_device: d_matrix on the contexts' device; only queues the work
 *     (the walk of ctx, then on the same stream the walk of other for the
 *     k-mers ctx lacks): no allocation, no synchronisation.
 * Joined views: a k-mer of ctx is kept when min_count <= its count <= max_count
 * and other_min <= its count in other <= other_max, all ends inclusive,
 * UINT32_MAX on an upper end: no upper bound.  min_count >= 1, min_count <=
 * max_count, other_min <= other_max, else FK_E_INVALID.  other_min = 0 admits
 * the k-mers other lacks: (other_min, other_max) = (0, 0) is "A minus B",
 * other_min >= 1 is "A intersect B", and (1, UINT32_MAX, 0, UINT32_MAX) gives
 * exactly fk_get_bin's keys and counts plus every k-mer's count in other.
 *   fk_bin_sizes_joined: kept k-mers per bin, all b bins (0 for bins owned by
 *     other ranks).
 *   fk_get_bin_joined: fk_get_bin_range's order and buffer rules: *n is always
 *     set, FK_E_RANGE when cap < *n or the bin is out of [0, b); keys, counts
 *     and other_counts may each be NULL; a bin of another rank answers 0. */
int fk_compare(fk_ctx *ctx, fk_ctx *other, uint64_t *matrix, size_t rows, size_t cols);
int fk_compare_device(fk_ctx *ctx, fk_ctx *other, void *d_matrix, size_t rows, size_t cols);
int fk_bin_sizes_joined(fk_ctx *ctx, fk_ctx *other, uint32_t min_count, uint32_t max_count,
                        uint32_t other_min, uint32_t other_max, uint64_t *kept_per_bin);
int fk_get_bin_joined(fk_ctx *ctx, fk_ctx *other, int32_t bin, uint32_t min_count, uint32_t max_count,
                      uint32_t other_min, uint32_t other_max, uint64_t *keys, uint32_t *counts,
                      uint32_t *other_counts, size_t cap, size_t *n);

/* ---- per-read abundance profiles (no reference counterpart) ----
 * The counts put back onto reads: for every read, how many of its k-mers are
 * solid and what their minimum, median and maximum abundance is (the inputs of
 * kmc_tools filter, normalize-by-median, abundance filters, error trimming and
 * contamination screens).
 * A read batch is CSR: bases = uint8[n_bases], the reads' sequence bytes back
 * to back with no separators; offsets = uint64[n_reads + 1], ascending,
 * offsets[0] = 0, offsets[n_reads] = n_bases; read i = bases[offsets[i],
 * offsets[i + 1]).  Reads may be empty or shorter than k.
 *   fk_reads_csr: host only.  Cuts FASTA or FASTQ text (FK_FORMAT_*) into a
 *     batch exactly as the count sees it.  FASTA: a read is what follows a
 *     header line (a non-empty line beginning with '>') up to the next one,
 *     the '\n' of its lines removed and every other byte kept ('\r', N,
 *     lowercase and IUPAC codes stay, as invalid positions); lines before the
 *     first header are no sequence.  FASTQ: the grammar of fk_set_input_format;
 *     the read is the sequence line (its '\r' under CRLF included), and with
 *     min_quality > 0 every base whose score is below it is 'N'; malformed
 *     input gives FK_E_INVALID, the message naming the first malformed record
 *     (0-based), with *n_reads / *n_bases those of the records before it.
 *     *n_reads and *n_bases are always set; bases == NULL or offsets == NULL:
 *     only they (a sizing call).  offsets holds cap_reads + 1 entries;
 *     FK_E_RANGE when cap_bases or cap_reads is too small.
 * Window p = bases[p, p + k) exists when it lies wholly inside one read and is
 * valid when it also holds only A/C/G/T.  Arrays are indexed by base position,
 * so read i's windows are counts[offsets[i] .. offsets[i] + max(len_i - k + 1, 0)).
 *   counts[p]: the count of the canonical k-mer of a valid window p, looked up
 *     exactly as fk_query does (either strand; 0 when absent or when another
 *     rank owns the k-mer's bin); 0 for every other position.
 *   valid[p] (may be NULL): 1 exactly for valid windows, the same on every
 *     rank; the ranks' counts sum to the job's answer.
 * Preconditions and errors are the lookups': a result of the sorted count
 * (FK_E_STATE without one, FK_E_INVALID for use_ht == 1).
 *   fk_read_counts_device: pointers on the context's device (d_counts
 *     uint32[n_bases], d_valid uint8[n_bases] or NULL; the kernel reads n_bases =
 *     offsets[n_reads] on the device); only queues on the context's stream: no
 *     allocation, no synchronisation.  d_bases 16-byte aligned loads fastest.
 *   fk_read_counts: host pointers, staged in chunks of FASTKMER_QUERY_CHUNK
 *     positions (each with its k - 1 halo bases and the offsets it touches);
 *     FK_E_INVALID for offsets that do not ascend from 0.
 * Per-read statistics over the valid windows, absent k-mers as count 0;
 * windows == 0: every field 0.  The count range is fk_get_bin_range's
 * (min_count >= 1, max_count = UINT32_MAX: no upper bound).
 *   fk_read_stats_of_counts_device: reduces position-indexed device arrays per
 *     read -- one rank's, or the ranks' summed by the caller; d_valid == NULL:
 *     every existing window is valid.  Needs only a context (its k), no result.
 *   fk_read_stats_device: fk_read_counts_device then the reduction, through the
 *     caller's scratch of fk_read_stats_scratch_bytes(n_bases) bytes (4-byte
 *     aligned); no allocation, no synchronisation.  Positions beyond a smaller
 *     scratch are left out of the statistics (nothing is written past it).
 *   fk_read_stats: host pointers, chunked on whole-read boundaries (a read
 *     longer than FASTKMER_QUERY_CHUNK positions gets a chunk of its own).
 *   The two forms that look counts up need every k-mer's count: on a context
 *   with n_ranks > 1 they return FK_E_INVALID (use fk_read_counts on every
 *   rank, sum, then fk_read_stats_of_counts_device). */
#define FK_READ_TILE 4096 /* positions per workgroup tile of the window kernel (tests aim read ends at it) */
typedef struct fk_read_stat { /* 32 bytes */
    uint32_t windows;  /* valid windows of the read */
    uint32_t hits;     /* of them, count in [min_count, max_count] */
    uint32_t min;      /* over the valid windows */
    uint32_t median;   /* element (windows - 1) / 2 of the ascending counts */
    uint32_t max;
    uint32_t reserved; /* 0 */
    uint64_t sum;      /* sum of the counts */
} fk_read_stat;
int fk_reads_csr(const uint8_t *text, size_t n, int32_t format, int32_t min_quality, int32_t quality_offset,
                 uint8_t *bases, size_t cap_bases, uint64_t *offsets, size_t cap_reads,
                 size_t *n_reads, size_t *n_bases);
int fk_read_counts_device(fk_ctx *ctx, const void *d_bases, const void *d_offsets, size_t n_reads,
                          void *d_counts, void *d_valid);
int fk_read_counts(fk_ctx *ctx, const uint8_t *bases, const uint64_t *offsets, size_t n_reads,
                   uint32_t *counts, uint8_t *valid);
int fk_read_stats_of_counts_device(fk_ctx *ctx, const void *d_counts, const void *d_valid, const void *d_offsets,
                                   size_t n_reads, uint32_t min_count, uint32_t max_count, void *d_stats);
int fk_read_stats_device(fk_ctx *ctx, const void *d_bases, const void *d_offsets, size_t n_reads,
                         uint32_t min_count, uint32_t max_count, void *d_scratch, size_t scratch_bytes, void *d_stats);
int fk_read_stats(fk_ctx *ctx, const uint8_t *bases, const uint64_t *offsets, size_t n_reads,
                  uint32_t min_count, uint32_t max_count, fk_read_stat *stats);
size_t fk_read_stats_scratch_bytes(size_t n_bases);

/* ---- export, import and the database file (no reference counterpart) ----
 * A counted result taken out of its context and put back: as arrays (a caller
 * holding (k-mer, count) pairs gets fk_query, fk_read_stats and fk_compare), or
 * as a binary file that outlives the process (jellyfish .jf, KMC .kmc_pre /
 * .kmc_suf).  Sorted count only: use_ht == 1 gives FK_E_INVALID.
 * The dense layout: the bins this rank owns in the order of its local bins
 * (ascending bin id under the default placement), each bin holding fk_get_bin's
 * keys (one word for k <= 32, (hi, lo) above) and counts; fk_bin_sizes gives the
 * cut points.
 *   fk_export: the whole result in that layout.  *n = the distinct k-mers, always
 *     set; FK_E_RANGE when cap < *n.  Reads the result only.
 *   fk_export_device: device pointers; only queues on the context's stream.
 *   fk_import: the inverse.  bin_sizes (host, all b entries) = the keys of every
 *     bin; a non-zero size for a bin this context does not own is FK_E_INVALID.
 *     Every key must be a k-mer (no bit above 2k - 1), canonical (not greater
 *     than its reverse complement), in the bin its position says, strictly above
 *     its predecessor in the bin, and have a count >= 1: else FK_E_INVALID, the
 *     message naming the bin, the index inside the bin and the reason, for the
 *     offending key with the smallest index.  A cell of 2^32 keys or more is
 *     FK_E_RANGE.  FK_E_STATE inside a job (between its first fk_ingest and
 *     fk_finish).  The arrays are copied: they are free once the call returns.
 *     On success the context is as fk_finish leaves it for every result call and
 *     a following job works; fk_get_stats reports distinct, kmers (the sum of the
 *     counts), buckets and fine_bits, every time and map figure 0.  On failure
 *     the context holds no result (result calls: FK_E_STATE).  As with a new job,
 *     no fk_compare_device of another context may be outstanding on this one.
 *   fk_import_device: d_keys / d_counts on the context's device, bin_sizes on the
 *     host; the work is queued on the context's stream and the call waits for it
 *     once, to read the verdict.
 * The file (version 1; little-endian, no timestamps: saving the same result
 * twice gives identical bytes):
 *   offset 0   8 bytes   magic "FKMERDB\0"
 *          8   u32       version = 1
 *         12   u32       header bytes (a multiple of 8): 72 + 16 * stored_bins
 *         16   6 x i32   k, m, bins (the clamped b), key_words (1 or 2), n_ranks,
 *                        rank of the saver
 *         40   u32       stored_bins;  44  u32  0
 *         48   3 x u64   distinct, kmers (the sum of the counts), checksum
 *         72   stored_bins x {u32 bin, u32 0, u64 distinct}: the non-empty bins
 *                        only, ascending
 *   header bytes         distinct x key_words x 8: the keys, bin after bin
 *   after the keys       distinct x 4: the counts
 * checksum = the wrapping 64-bit sum of mix(v ^ (i * 0x9E3779B97F4A7C15)) over the
 * key words v (i = the word's index in the key section) and the counts (i = 2^63
 * + the count's index), mix = splitmix64's finaliser.  x, sequence_type and the
 * requested B are not stored: the bin function needs only k, m and b.
 *   fk_db_info_read: host only, and the only parser of the file's bytes.
 *     Validates the magic and the version, header bytes against stored_bins, the
 *     bins ascending, unique and below `bins`, their sizes non-zero and summing
 *     to distinct, key_words against k (FK_E_INVALID), and the file's size
 *     against the header (FK_E_IO: "truncated" or "trailing bytes").
 *   fk_save: export, checksum on the device, copy out through two pinned windows
 *     while the previous one is written; <path>.tmp, then rename.  FK_E_IO with
 *     errno's text on a file error.  An empty result saves a header with no bins.
 *   fk_load: the header checked against the context -- k, m, bins, key_words
 *     (FK_E_INVALID naming the field) and every stored bin owned by it: a file
 *     saved by rank r of n loads into a context of the same rank and placement,
 *     and into a one-rank context -- then the sections streamed in and fk_import's
 *     checks; a checksum or kmers mismatch is FK_E_INVALID. */
typedef struct fk_db_info {
    int32_t k, m, bins, key_words, n_ranks, rank, version, stored_bins;
    uint64_t distinct, kmers, checksum, file_bytes;
} fk_db_info;
int fk_export(fk_ctx *ctx, uint64_t *keys, uint32_t *counts, size_t cap, size_t *n);
int fk_export_device(fk_ctx *ctx, void *d_keys, void *d_counts, size_t cap, size_t *n);
int fk_import(fk_ctx *ctx, const uint64_t *keys, const uint32_t *counts, const uint64_t *bin_sizes);
int fk_import_device(fk_ctx *ctx, const void *d_keys, const void *d_counts, const uint64_t *bin_sizes);
int fk_db_info_read(const char *path, fk_db_info *out);
int fk_save(fk_ctx *ctx, const char *path);
int fk_load(fk_ctx *ctx, const char *path);
/* Measurement hook: the last fk_save / fk_load / fk_import* of the context in ms -- out[0] wall,
 * out[1] export + checksum (save) or H2D of the arrays (device events), out[2] the copy out (save: the
 * host's waits for its windows) or the file reads (load), out[3] the file writes, out[4..7) the
 * import's verify, cell offsets and bucket tables (device events), out[7] = 0. */
int fk_debug_store_ms(const fk_ctx *ctx, double out[8]);

/* ---- test hook (no reference counterpart) ----
 * One bucket through the wave-tier count kernel on `device`: the n keys
 * (k <= 32: one word each, n <= 512; 33 <= k <= 63: (hi, lo) pairs, n <= 256)
 * must lie in cells [c0, c1) of F cell bits (cell = top F bits of the 2k-bit
 * key); slots = table slots per bucket, the product's (640, or 384 for k > 32).
 * Writes the distinct keys ascending and their counts, *n_out of them.  Lets
 * tests drive adversarial buckets (every key in one rank group, keys over all
 * groups) that FASTA inputs cannot aim at. */
int fk_debug_wave_count(int32_t device, int32_t k, int32_t F, uint32_t c0, uint32_t c1, int32_t slots,
                        const uint64_t *keys, uint32_t n, uint64_t *out_keys, uint32_t *out_counts,
                        uint32_t *n_out);
/* The same for a bucket of weighted keys, as the fold of a landed piece leaves
 * them (2k <= 60: bits [2k, 2k + 4) of a key hold weight - 1, the key stands
 * for 1..15 occurrences of its k-mer): the counts are sums of weights.  A key
 * with bits above its k-mer where there is no weight field (k = 31), or above
 * the field, is rejected (FK_E_RANGE). */
int fk_debug_wave_count_w(int32_t device, int32_t k, int32_t F, uint32_t c0, uint32_t c1, int32_t slots,
                          const uint64_t *keys, uint32_t n, uint64_t *out_keys, uint32_t *out_counts,
                          uint32_t *n_out);
/* The fold of the last fk_finish (one rank's staged pieces, k <= 30; FASTKMER_FOLD
 * = 0 off, 1 by a sample of the first piece, 2 every eligible piece): out[0] =
 * pieces folded, out[1] = their k-mers, out[2] = the weighted entries they were
 * folded to, out[3] = the sample's entries per million k-mers (0: no sample). */
int fk_debug_fold_stats(const fk_ctx *ctx, uint64_t out[4]);
/* The staged count -- the bucket cut, every tier and its fallbacks, the fold -- over
 * staged pieces the caller supplies, on a context created as usual (k <= 63, one
 * rank, no communicator, no job open).  F = cell bits, 1 .. min(15, 2k); the
 * super-cell bits follow from F as in a job.  np = 1 .. 5 pieces (k > 32: 1 .. 4).
 * keys[p] (host) = piece p's keys laid out by (local bin, cell): one word for
 * k <= 32, (hi, lo) pairs above; cell_counts[p] = its keys per cell, bins << F
 * words.  weighted (2k <= 60 only): bits [2k, 2k + 4) of a key hold weight - 1
 * <= 14.  Every piece whose bit is set in fold_mask (2k <= 60 only) is folded first
 * by the job's own fold, under FASTKMER_DEBUG_FOLD_WMAX.  Every key must lie in the
 * cell and the bin its position says and have nothing above its k-mer but the
 * weight (FK_E_RANGE); the word ~0 is refused too: it marks an empty table slot,
 * and is a k-mer only at k = 32 (all T) or, under weight 15, at k = 30 (all T) --
 * canonical k-mers are never all T.  Afterwards the context is as fk_finish leaves
 * it: fk_bin_sizes, fk_get_bin, fk_get_stats (kmers = the sum of the weights),
 * fk_debug_fold_stats work, and so does a following job. */
int fk_debug_count_pieces(fk_ctx *ctx, int32_t F, int32_t np, const uint64_t *const *keys,
                          const uint64_t *const *cell_counts, int32_t weighted, uint32_t fold_mask);
/* The last tiered count's census, from figures its driver reads anyway: out[0] =
 * mid-tier buckets (513 .. 1024 keys, k <= 32) its first kernel handed on to the
 * 1024-key kernel, out[1] / out[2] = split buckets left to the block kernel / LDS
 * sort (at most 2048 keys) and to the big table or the streaming path (above),
 * out[3] = buckets that ended on the streaming path, out[4] = the mid tier's first
 * kernel (0 none, 1 key ranges, 2 whole buckets on the 512-key table); out[5..8) = 0. */
int fk_debug_tier_stats(const fk_ctx *ctx, uint64_t out[8]);
/* Staged piece p of the last counted job as the count read it (folded, if it was):
 * out_cb = the exclusive scan of its keys per cell, (bins << F) + 1 words, the last
 * one the piece's keys; out_keys (or NULL) = those keys.  Valid until the next job. */
int fk_debug_staged_piece(fk_ctx *ctx, int32_t p, uint64_t *out_keys, uint64_t *out_cb);
/* Device allocations, pinned host allocations, events and streams currently owned by the library's
 * contexts and calls in this process (a communicator's own are not included, nor a scan workspace --
 * at most two device allocations per context, made inside the scans).  Test hook. */
int fk_debug_live_resources(uint64_t out[4]);

/* ---- test hooks of the failure semantics (no reference counterpart) ----
 * fk_debug_comm_hold queues, on every stream the context's collectives run on,
 * a one-thread kernel that spins on a host-mapped flag (it ends by itself after
 * max_seconds), so that the next collective call waits on a stream that does
 * not drain -- what a rank blocked by a dead peer sees.  fk_debug_comm_release
 * sets the flag (callable from another thread while a collective is waiting);
 * fk_destroy releases it too. */
int fk_debug_comm_hold(fk_ctx *ctx, int32_t max_seconds);
int fk_debug_comm_release(fk_ctx *ctx);
/* 1 while the context's comm stream has not drained (e.g. still held), else 0. */
int fk_debug_comm_held(fk_ctx *ctx);

/* Test hook: the 128-bit wave tier (33 <= k <= 63) dedupes on 64-bit key
 * fingerprints and checks every key against its slot's claimer; a shared
 * fingerprint sends the bucket to an exact count from LDS.  This cuts
 * the fingerprints of `device` to their low `bits` bits (0: whole, the
 * product), so that tests drive that path on every bucket. */
int fk_debug_fingerprint_bits(int32_t device, int32_t bits);

/* Measurement hook: per-phase wave cycles of the fused map kernel summed over
 * its launches since the last reset (out[0..16)); only a library built with
 * -DFK_PROBES records them (FK_E_STATE otherwise). */
int fk_debug_map_cycles(uint64_t *out16, int32_t reset);

/* Measurement hook: after the fk_map / fk_finish of a FASTQ job, *ms = the device-event time summed
 * over the job's normalise launches (each the stage's two kernels and the memset before them),
 * *launches = how many there were. */
int fk_debug_fastq_ms(fk_ctx *ctx, double *ms, uint64_t *launches);

/* ---- bin-signature diagnostics (executeFindBinSignaturesJob, SBKC:956-986) ----
 * fk_signature_counts: after the final fk_ingest (the input is left in place,
 *   fk_map may follow), d_counts[v] (device memory of the ctx device, uint64)
 *   = super-k-mers with signature v over this rank's input -- getBinSignatures
 *   (SBKC:772-917); v = 4^m when every m-mer of the window is forbidden.  It
 *   needs fk_signature_slots(ctx) = 4^m + 1 entries.  Across ranks, sum the
 *   arrays (an all-reduce: the reduceByKey of SBKC:984) before writing.
 * fk_write_bin_signatures: saveBinSignatures (SBKC:920-953) for the bins this
 *   rank owns: <out_dir>/bin_signatures<b>.txt, "<signature>\t<count>\n" lines
 *   (longToString: 31 characters, PKG:616-634) in ascending signature order,
 *   then "Total\t<sum>\n"; bins without signatures get no file. */
uint64_t fk_signature_slots(const fk_ctx *ctx);
int fk_signature_counts(fk_ctx *ctx, void *d_counts, uint64_t n_counts);
int fk_write_bin_signatures(fk_ctx *ctx, const void *d_counts, uint64_t n_counts, const char *out_dir);
/* The whole job on one rank (n_ranks == 1, or each rank's own input unmerged):
 * fk_signature_counts into a library-owned buffer, then fk_write_bin_signatures. */
int fk_find_bin_signatures(fk_ctx *ctx, const char *out_dir);

#ifdef __cplusplus
}
#endif
#endif /* FASTKMER_H */
