// fk_api.cpp -- C-ABI of the MI355X k-mer counter (include/fastkmer.h).
//
// Host orchestration of the device pipeline in fk_kernels.hip.  Replaces the
// body of SparkBinKmerCounter.executeJob (SparkBinKmerCounter.scala:989-1046):
// the map closure, the reduceByKey shuffle and the reduce closure.  All device
// memory is owned by the context (fk_ctx.h) and reused across calls (grow-only);
// the calls that only read a finished result are in fk_views.cpp.
#include <errno.h>
#include <fcntl.h>
#include <unistd.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <sys/stat.h>

#include <unordered_map>
#include <chrono>
#include <memory>
#include <cstdlib>
#include <cstring>
#include <thread>

#include "fk_ctx.h"
#include "fk_split.h"

static thread_local std::string g_err;  // fk_last_error's message
int fk::set_err(int code, const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

namespace {
// Counts records and k-mers per part into pb.rec / pb.kmer (device) and keeps
// what part_scatter needs.
int part_count(PartBufs &pb, const RecSrc &src, int mode, uint32_t G, const uint32_t *table, uint32_t nparts,
               ScanWorkspace &ws, hipStream_t s) {
    pb.nparts = nparts;
    pb.src = src;
    pb.global = nparts > PART_MAX;
    FK_TRY(ensure(pb.rec, ((uint64_t)nparts + 1) * 8));
    FK_TRY(ensure(pb.kmer, ((uint64_t)nparts + 1) * 8));
    FK_TRY(ensure(pb.off, ((uint64_t)nparts + 1) * 8));
    if (pb.global) {
        HIP_TRY(hipMemsetAsync(pb.rec.p, 0, ((uint64_t)nparts + 1) * 8, s));
        HIP_TRY(hipMemsetAsync(pb.kmer.p, 0, ((uint64_t)nparts + 1) * 8, s));
        HIP_TRY(launch_part_hist_global(src, mode, G, table, nparts, pb.rec.as<uint64_t>(), pb.kmer.as<uint64_t>(), s));
        HIP_TRY(scan_excl_sum_u64(pb.rec.as<uint64_t>(), pb.off.as<uint64_t>(), nparts, pb.off.as<uint64_t>() + nparts,
                                  ws, s));
        return FK_OK;
    }
    const uint32_t nwg = src.nrec ? part_workgroups(src) : 0u;
    const uint64_t n = (uint64_t)nparts * nwg;
    FK_TRY(ensure(pb.H, n * 4));
    FK_TRY(ensure(pb.K, n * 4));
    const uint64_t nt = (uint64_t)nparts * part_segments(nwg);
    FK_TRY(ensure(pb.Hs, n * 8));
    FK_TRY(ensure(pb.Ts, (nt + 1) * 8));
    FK_TRY(ensure(pb.KT, nt * 8));
    if (n) {
        HIP_TRY(launch_part_hist(src, mode, G, table, nparts, pb.H.as<uint32_t>(), pb.K.as<uint32_t>(), s));
        HIP_TRY(launch_part_segsum(pb.H.as<uint32_t>(), pb.K.as<uint32_t>(), nparts, nwg, pb.Ts.as<uint64_t>(),
                                   pb.KT.as<uint64_t>(), s));
        HIP_TRY(scan_excl_sum_u64(pb.Ts.as<uint64_t>(), pb.Ts.as<uint64_t>(), nt, pb.Ts.as<uint64_t>() + nt, ws, s));
        HIP_TRY(launch_part_segfill(pb.H.as<uint32_t>(), pb.Ts.as<uint64_t>(), nparts, nwg, pb.Hs.as<uint64_t>(), s));
        HIP_TRY(launch_part_totals(pb.Ts.as<uint64_t>(), pb.KT.as<uint64_t>(), nparts, nwg, pb.rec.as<uint64_t>(),
                                   pb.kmer.as<uint64_t>(), pb.off.as<uint64_t>(), s));
    } else {
        HIP_TRY(hipMemsetAsync(pb.rec.p, 0, ((uint64_t)nparts + 1) * 8, s));
        HIP_TRY(hipMemsetAsync(pb.kmer.p, 0, ((uint64_t)nparts + 1) * 8, s));
        HIP_TRY(hipMemsetAsync(pb.off.p, 0, ((uint64_t)nparts + 1) * 8, s));
    }
    return FK_OK;
}

// Writes the records grouped by part (parts in order) into out.
int part_scatter(PartBufs &pb, int mode, uint32_t G, const uint32_t *table, uint64_t *out, hipStream_t s) {
    if (!pb.src.nrec) return FK_OK;
    if (pb.global) {
        FK_TRY(ensure(pb.cursor, ((uint64_t)pb.nparts + 1) * 8));
        HIP_TRY(hipMemsetAsync(pb.cursor.p, 0, ((uint64_t)pb.nparts + 1) * 8, s));
        HIP_TRY(launch_part_scatter_global(pb.src, mode, G, table, pb.nparts, pb.off.as<uint64_t>(),
                                           pb.cursor.as<uint64_t>(), out, s));
        return FK_OK;
    }
    HIP_TRY(launch_part_scatter(pb.src, mode, G, table, pb.nparts, pb.Hs.as<uint64_t>(), out, s));
    return FK_OK;
}

double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// -DFK_PROBES library, FASTKMER_HOST_TRACE=1: host timestamps of the count's steps on stderr (where
// the GPU waits on the host)
static void htrace(const char *what) {
#ifdef FK_PROBES
    static const bool on = getenv("FASTKMER_HOST_TRACE") && getenv("FASTKMER_HOST_TRACE")[0] == '1';
    if (on) fprintf(stderr, "htrace %.3f %s\n", now_ms(), what);
#else
    (void)what;
#endif
}

constexpr int FUSED_NT = 512;  // threads per fused map workgroup (256-thread tiles measured 2.5 vs 1.1 ms per GB)
constexpr uint32_t CHUNK_RECORDS = 16384;  // records per expansion workgroup (never spans two bins)

}  // namespace

// ---------------------------------------------------------------------------
// host-only helpers
// ---------------------------------------------------------------------------

FK_EXPORT int fk_abi_version(void) { return FK_ABI_VERSION; }

// The measurement probes' settings (-DFK_PROBES); the product library has none.
#ifdef FK_PROBES
static int bucket_probe_phase(const fk_ctx *c) { return c->dbg_phase; }  // 99: none
static int fused_probe(const fk_ctx *c) { return c->fused_probe; }
static bool map_split(const fk_ctx *c) { return c->split_map && !c->fused_probe; }
#else
static int bucket_probe_phase(const fk_ctx *) { return 99; }
static int fused_probe(const fk_ctx *) { return 0; }
static bool map_split(const fk_ctx *) { return false; }
#endif

// Host waits on work that may depend on the exchange (the comm stream, the staging stream that waits
// for a step's transfer, events behind them): with a communicator they are bounded (Comm::wait: RCCL
// polls, times out after FASTKMER_COMM_TIMEOUT_S and aborts the communicator) and fail with FK_E_COMM.
static int comm_sync(fk_ctx *c, hipStream_t st) {
    if (!c->comm) {
        HIP_TRY(hipStreamSynchronize(st));
        return FK_OK;
    }
    std::string err;
    if (c->comm->wait(st, err)) return set_err(FK_E_COMM, "%s", err.c_str());
    return FK_OK;
}
static int comm_event_sync(fk_ctx *c, hipEvent_t ev) {
    if (!c->comm) {
        HIP_TRY(hipEventSynchronize(ev));
        return FK_OK;
    }
    std::string err;
    if (c->comm->wait_event(ev, err)) return set_err(FK_E_COMM, "%s", err.c_str());
    return FK_OK;
}

FK_EXPORT const char *fk_last_error(void) { return g_err.c_str(); }

FK_EXPORT int fk_config_init(fk_config *c) {
    if (!c) return set_err(FK_E_INVALID, "null config");
    // LocalTestKmerCounter.scala:20-33 defaults
    c->k = 20;
    c->m = 4;
    c->x = 3;
    c->B = 2000;
    c->use_ht = 0;
    c->sequence_type = 0;
    c->write = 0;
    c->n_ranks = 1;
    c->rank = 0;
    c->device = -1;
    return FK_OK;
}

FK_EXPORT int32_t fk_clamped_bins(int32_t m, int32_t B) { return clamp_bins(m, B); }

FK_EXPORT int fk_config_validate(const fk_config *c) {
    if (!c) return set_err(FK_E_INVALID, "null config");
    if (c->k < 1 || c->k > 64) return set_err(FK_E_INVALID, "k=%d out of range [1, 64]", c->k);
    if (c->m < 1 || c->m > 15)
        return set_err(FK_E_INVALID, "m=%d out of range [1, 15] (m >= 16 overflows Int shifts, SBKC:50)", c->m);
    if (c->m > c->k) return set_err(FK_E_INVALID, "m=%d must not exceed k=%d", c->m, c->k);
    if (c->B < 1) return set_err(FK_E_INVALID, "B=%d must be >= 1 (hash_to_bucket divides by B)", c->B);
    if (c->use_ht != 0 && c->use_ht != 1) return set_err(FK_E_INVALID, "use_ht must be 0 or 1");
    if (c->use_ht == 0 && c->x < 1)
        return set_err(FK_E_INVALID,
                       "x=%d: the sorted path needs x >= 1 (extractKXmers indexes R(runLength-1), SBKC:435/508)",
                       c->x);
    if (c->sequence_type != 0 && c->sequence_type != 1)
        return set_err(FK_E_INVALID, "sequence_type must be 0 (short) or 1 (long)");
    if (c->n_ranks < 1) return set_err(FK_E_INVALID, "n_ranks must be >= 1");
    if (c->rank < 0 || c->rank >= c->n_ranks) return set_err(FK_E_INVALID, "rank %d out of [0, %d)", c->rank, c->n_ranks);
    const int32_t bc = clamp_bins(c->m, c->B);
    if ((uint32_t)bc > REC_BIN_MASK + 1u)
        return set_err(FK_E_INVALID, "b = min(4^m, B) = %d exceeds the record header limit %u", bc, REC_BIN_MASK + 1u);
    return FK_OK;
}

FK_EXPORT int fk_output_dir(const fk_config *c, const char *output_path, const char *prefix, char *out, size_t cap) {
    if (!c || !out) return set_err(FK_E_INVALID, "null argument");
    // test/package.scala:33 (debug == false)
    const int n = snprintf(out, cap, "%s%sk%d_m%d_x%d_b%d_s%d", output_path ? output_path : "", prefix ? prefix : "",
                           c->k, c->m, c->x, clamp_bins(c->m, c->B), c->sequence_type);
    if (n < 0 || (size_t)n >= cap) return set_err(FK_E_RANGE, "output buffer too small (%d bytes needed)", n + 1);
    return FK_OK;
}

FK_EXPORT size_t fk_record_bytes_for_k(int32_t k) { return k <= 32 ? 16 : 24; }

FK_EXPORT uint64_t fk_synth_record_bytes(int32_t read_len) { return (uint64_t)read_len + 14; }

static SynthParams make_synth(uint64_t first_read, uint64_t n_reads, int32_t read_len, uint64_t genome_len,
                              uint64_t seed, double err_rate, double n_rate) {
    SynthParams p;
    p.first_read = first_read;
    p.n_reads = n_reads;
    p.genome_len = genome_len;
    p.seed = seed;
    p.read_len = (uint32_t)read_len;
    p.rec_bytes = (uint32_t)read_len + 14;
    const double two64 = 18446744073709551616.0;
    p.err_thresh = (uint64_t)(err_rate * two64 * 0.999999);
    p.n_thresh = (uint64_t)(n_rate * two64 * 0.999999);
    return p;
}

FK_EXPORT int fk_synth_fasta_host(uint8_t *out, uint64_t first_read, uint64_t n_reads, int32_t read_len,
                                  uint64_t genome_len, uint64_t seed, double err_rate, double n_rate) {
    if (!out || read_len < 1 || genome_len < 1) return set_err(FK_E_INVALID, "bad synth arguments");
    const SynthParams p = make_synth(first_read, n_reads, read_len, genome_len, seed, err_rate, n_rate);
    const uint64_t nb = n_reads * p.rec_bytes;
    for (uint64_t i = 0; i < nb; ++i) out[i] = synth_byte(p, i);
    return FK_OK;
}

// ---------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------

// What the environment sets in a new context.
static void read_env(fk_ctx *c) {
    // The product library reads thirteen variables: three sizes of the streamed input, the fold's gate
    // (FASTKMER_FOLD), the lookups' staging chunk (FASTKMER_QUERY_CHUNK, read by every fk_query /
    // fk_query_sequence call) and eight test
    // hooks that steer small inputs onto paths only large or adversarial inputs reach (all
    // result-preserving).  Timing probes that alter results exist only in a library built with
    // -DFK_PROBES (python -m fastkmer_amd.build --probes).
    auto env = [](const char *name) -> const char * {
        const char *v = getenv(name);
        return v && v[0] ? v : nullptr;
    };
    if (const char *v = env("FASTKMER_PIECE_BYTES")) {  // piece size of a streamed job (1 GB with a communicator)
        c->piece_bytes = std::max(1ull << 16, strtoull(v, nullptr, 10));
        c->piece_bytes_set = true;
    }
    if (const char *v = env("FASTKMER_PIECE_CUTS")) {  // staged piece ends as job fractions, e.g. "0.4,0.7,0.9"
        c->st_cuts.clear();
        c->xst_cuts.clear();
        for (const char *q = v; *q;) {
            char *e = nullptr;
            const double f = strtod(q, &e);
            if (e == q) break;
            if (f > 0.0 && f < 1.0 && c->st_cuts.size() < STAGE_MAXP - 1) c->st_cuts.push_back(f), c->xst_cuts.push_back(f);
            c->cuts_env = true;
            q = *e == ',' ? e + 1 : e;
        }
    }
    if (const char *v = env("FASTKMER_INGEST_SEG")) c->ingest_seg = std::max(1ull << 16, strtoull(v, nullptr, 10));
    if (const char *v = env("FASTKMER_DEBUG_LARGE_BUCKETS")) c->force_large = v[0] == '1';
    if (const char *v = env("FASTKMER_DEBUG_CELL_TARGET")) c->cell_target = (uint32_t)atoi(v);
    if (const char *v = env("FASTKMER_DEBUG_MID_PARTS")) c->mid_parts = atoi(v);  // test hook: 1 / 2 / 0
    if (const char *v = env("FASTKMER_DEBUG_SPLIT_RETRY")) c->split_retry = v[0] == '1';  // test hook
    if (const char *v = env("FASTKMER_DEBUG_SPECTRUM_WIDE")) c->spectrum_wide = v[0] == '1';  // test hook
    if (const char *v = env("FASTKMER_FOLD")) c->fold_mode = std::clamp(atoi(v), 0, 2);
    if (const char *v = env("FASTKMER_DEBUG_FOLD_WMAX"))  // test hook
        c->fold_wmax = (uint32_t)std::clamp(atoi(v), 1, (int)WKEY_WMAX);
    if (const char *v = env("FASTKMER_X2_L1")) c->x2_l1 = atoi(v);
    if (const char *v = env("FASTKMER_FUSED")) c->fused = atoi(v);
#ifdef FK_PROBES
    if (const char *v = env("FASTKMER_DEBUG_PHASE")) c->dbg_phase = atoi(v);
    if (const char *v = env("FASTKMER_FUSED_PROBE")) c->fused_probe = atoi(v);
    if (const char *v = env("FASTKMER_SPLIT_MAP")) c->split_map = atoi(v);
#endif
}

FK_EXPORT int fk_create(const fk_config *cfg, fk_ctx **out) {
    if (!out) return set_err(FK_E_INVALID, "null output pointer");
    *out = nullptr;
    FK_TRY(fk_config_validate(cfg));
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        return set_err(FK_E_DEVICE, "no HIP device available (%s): the k-mer counter runs on MI355X only",
                       hipGetErrorString(e));
    }
    // any failure below leaves through this owner: fk_destroy takes a context however far it got
    std::unique_ptr<fk_ctx, void (*)(fk_ctx *)> ctx(new fk_ctx(), fk_destroy);
    fk_ctx *c = ctx.get();
    c->cfg = *cfg;
    c->Bc = clamp_bins(cfg->m, cfg->B);
    c->G = (uint32_t)cfg->n_ranks;
    c->nlb = (uint32_t)((c->Bc - cfg->rank + (int)c->G - 1) / (int)c->G);
    if (cfg->rank >= c->Bc) c->nlb = 0;
    c->W = cfg->k <= 32 ? 2 : 3;
    c->KW = cfg->k <= 32 ? 1 : 2;
    c->fm = make_fastmod((uint32_t)c->Bc);
    read_env(c);
    if (cfg->device >= 0) {
        if (cfg->device >= ndev) {
            c->device = -1;  // none to select on the way out
            return set_err(FK_E_DEVICE, "device %d out of range (%d devices)", cfg->device, ndev);
        }
        c->device = cfg->device;
    } else {
        (void)hipGetDevice(&c->device);
    }
    DeviceGuard dg_(c->device);  // the caller's current device is restored on return
    {
        int cur = -1;
        if (hipGetDevice(&cur) != hipSuccess || cur != c->device) {
            (void)hipGetLastError();
            return set_err(FK_E_DEVICE, "cannot select device %d", c->device);
        }
    }
    // the streams and events (roles: DESIGN.md, "The context: what lives how long"); an event is timed
    // unless it only orders streams
    constexpr unsigned ORDER = hipEventDisableTiming;
    e = c->stream.create();
    if (e != hipSuccess) return set_err(FK_E_DEVICE, "hipStreamCreate: %s", hipGetErrorString(e));
    int least = 0, greatest = 0;
    const bool prio = hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess;
    e = c->copy_stream.create();
    if (e == hipSuccess) e = c->seg_ev.create(ORDER);
    if (e == hipSuccess) e = c->xstage.create();
    if (e == hipSuccess) e = c->xstage_ev.create(ORDER);
    if (e == hipSuccess) e = c->tier_side.create(prio ? &greatest : nullptr);
    for (int i = 0; i < 4 && e == hipSuccess; ++i) e = c->side_ev[i].create(ORDER);
    for (int i = 0; i < 2 && e == hipSuccess; ++i) e = c->h2d_ev[i].create();
    if (e != hipSuccess) return set_err(FK_E_DEVICE, "copy stream / events: %s", hipGetErrorString(e));
    for (int i = 0; i < 12 && e == hipSuccess; ++i) e = c->ev[i].create();
    for (Event *ev : {&c->tier_ev, &c->pin_up_ev, &c->cmp_ev})
        if (e == hipSuccess) e = ev->create(ORDER);
    for (int i = 0; i < 4 * STAGE_MAXP && e == hipSuccess; ++i) e = c->st_ev[i].create();
    if (e != hipSuccess) return set_err(FK_E_DEVICE, "hipEventCreate: %s", hipGetErrorString(e));
    *out = ctx.release();
    return FK_OK;
}

// Every member that holds a GPU handle frees it when the context is deleted (fk_ctx.h); what is left to do
// here is to let the work that may still use them end.
FK_EXPORT void fk_destroy(fk_ctx *c) {
    if (!c) return;
    DeviceGuard dg_(c->device);
    if (c->hold_flag.p) __atomic_store_n(c->hold_flag.as<uint32_t>(), 1u, __ATOMIC_RELEASE);  // a test's held streams drain
    // the copy, the map and count, staged expansions of an ingest without fk_finish, the heavy tiers of a
    // count that failed half way, the exchange
    for (hipStream_t s : {(hipStream_t)c->copy_stream, (hipStream_t)c->stream, (hipStream_t)c->xstage,
                          (hipStream_t)c->tier_side, (hipStream_t)c->comm_stream})
        if (s) (void)hipStreamSynchronize(s);
    delete c->comm;
    delete c;
}

FK_EXPORT int fk_set_stream(fk_ctx *c, void *s) {
    if (!c) return set_err(FK_E_INVALID, "null ctx");
    DeviceGuard dg_(c->device);
    if (c->stream.own) (void)hipStreamSynchronize(c->stream);
    c->stream.borrow((hipStream_t)s);  // the caller's: never destroyed here
    return FK_OK;
}

FK_EXPORT size_t fk_record_bytes(const fk_ctx *c) { return c ? (size_t)c->W * 8 : 0; }
FK_EXPORT int32_t fk_num_bins(const fk_ctx *c) { return c ? c->Bc : 0; }

void reset_results(fk_ctx *c) {
    c->mapped = false;
    c->have_result = false;
    c->gapped = c->dense_ready = false;
    c->distinct = 0;
    c->h_bin_off.clear();
}

// A new map or count opens: no result, no records, fresh statistics.
static void new_result(fk_ctx *c) {
    reset_results(c);
    c->stats = fk_stats{};
    c->nrec = c->nkmers = 0;
    c->rec_tiled = false;
}

// A job begins (the one place): its state from scratch, the last result gone, and for a FASTQ input the
// stage's counters zeroed on the map stream.  The callers then set what is particular to their kind of
// input.  The format is the job's from here on.
static int begin_job(fk_ctx *c, bool fastq) {
    c->job = fk_ctx::Job{};
    reset_results(c);
    c->job.job_open = true;
    c->job.fq_job = fastq;
    if (!fastq) return FK_OK;
    FK_TRY(ensure(c->fq_info, 32));
    if (c->fq_pin.ensure(32)) return set_err(FK_E_NOMEM, "hipHostMalloc(32) failed");
    HIP_TRY(hipMemsetAsync(c->fq_info.p, 0, 32, c->stream));
    return FK_OK;
}

// A job's count is done (or given up): its staged pieces are no more, a later count takes the whole input.
static void end_pieces(fk_ctx *c) { static_cast<fk_ctx::Pieces &>(c->job) = fk_ctx::Pieces{}; }

static float ev_ms(hipEvent_t a, hipEvent_t b) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, a, b) != hipSuccess) {
        (void)hipGetLastError();
        return 0.f;
    }
    return ms;
}

constexpr size_t PIN_CHUNK = 32ull << 20;  // pinned staging buffer (x2) for pageable sources

// Grows b to at least `bytes`, keeping its first `keep` bytes (stream-ordered copy).
static int grow_keep(DevBuf &b, size_t bytes, size_t keep, hipStream_t s) {
    if (b.bytes >= bytes) return FK_OK;
    DevBuf g;
    FK_TRY(ensure(g, std::max<size_t>(bytes, 2 * b.bytes)));
    if (keep && b.p) HIP_TRY(hipMemcpyAsync(g.p, b.p, std::min(keep, b.bytes), hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    b = std::move(g);
    return FK_OK;
}

// ---- FASTQ input: the device stage in front of the FASTA parsers (fk_fastq.inc)

FK_EXPORT int fk_set_input_format(fk_ctx *c, int32_t format, int32_t min_quality, int32_t quality_offset) {
    if (!c) return set_err(FK_E_INVALID, "null ctx");
    if (c->job.job_open) return set_err(FK_E_STATE, "fk_set_input_format inside a job (after its first fk_ingest)");
    if (format != FK_FORMAT_FASTA && format != FK_FORMAT_FASTQ) return set_err(FK_E_INVALID, "unknown input format %d", format);
    if (quality_offset != 33 && quality_offset != 64)
        return set_err(FK_E_INVALID, "quality_offset must be 33 or 64, got %d", quality_offset);
    if (min_quality < 0 || min_quality > 93) return set_err(FK_E_INVALID, "min_quality must be in 0..93, got %d", min_quality);
    if (format == FK_FORMAT_FASTQ && c->cfg.sequence_type != 0)
        return set_err(FK_E_INVALID, "FASTQ input needs sequence_type 0 (short reads)");
    c->in_format = format;
    c->fq_min_q = min_quality;
    c->fq_q_off = quality_offset;
    return FK_OK;
}

FK_EXPORT int fk_input_format(const fk_ctx *c, int32_t *format, int32_t *min_quality, int32_t *quality_offset) {
    if (!c) return set_err(FK_E_INVALID, "null ctx");
    if (format) *format = c->in_format;
    if (min_quality) *min_quality = c->fq_min_q;
    if (quality_offset) *quality_offset = c->fq_q_off;
    return FK_OK;
}

FK_EXPORT int fk_fastq_info(fk_ctx *c, uint64_t out[3]) {
    if (!c || !out) return set_err(FK_E_INVALID, "null argument");
    if (!c->fq_have_info) return set_err(FK_E_STATE, "fk_fastq_info before the fk_map / fk_finish of a FASTQ job");
    for (int i = 0; i < 3; ++i) out[i] = c->fq_out[i];
    return FK_OK;
}

FK_EXPORT int fk_debug_fastq_ms(fk_ctx *c, double *ms, uint64_t *launches) {
    if (!c || !ms || !launches) return set_err(FK_E_INVALID, "null argument");
    if (!c->fq_have_info || c->job.job_open) return set_err(FK_E_STATE, "fk_debug_fastq_ms before the fk_map / fk_finish of a FASTQ job");
    DeviceGuard dg_(c->device);
    double sum = 0.0;
    for (size_t i = 0; i + 1 < c->job.fq_nev; i += 2) sum += ev_ms(c->fq_evs[i], c->fq_evs[i + 1]);
    *ms = sum;
    *launches = c->job.fq_nev / 2;
    return FK_OK;
}

FK_EXPORT int fk_fastq_frontier(const uint8_t *buf, size_t n, size_t *off) {
    if ((!buf && n) || !off) return set_err(FK_E_INVALID, "null argument");
    *off = (size_t)fastq_frontier_scan([buf](uint64_t p) { return buf[p]; }, 0, n);
    return FK_OK;
}

// Queues the normalisation of the record-aligned range [a, b) of fasta_own on the map stream
// (src: the bytes come from src[a, b), a borrowed input); final_: the input ends at b.
static int fq_normalise(fk_ctx *c, const uint8_t *src, uint64_t a, uint64_t b, bool final_) {
    if (b <= a) return FK_OK;
    if (b - a >= (1ull << 32))
        return set_err(FK_E_INVALID, "FASTQ: %llu bytes in one normalise range (a record, or a device input, of 4 GiB or more)",
                       (unsigned long long)(b - a));
    FK_TRY(ensure(c->fq_ws, fastq_ws_bytes(b - a)));
    HIP_TRY(ensure_events(c->fq_evs, c->job.fq_nev + 2));
    HIP_TRY(hipEventRecord(c->fq_evs[c->job.fq_nev], c->stream));
    HIP_TRY(launch_fastq_normalise(c->fasta_own.as<uint8_t>(), src, a, b, final_ ? 1 : 0, c->fq_min_q, c->fq_q_off,
                                   c->fq_ws.p, c->fq_info.as<unsigned long long>(), c->stream));
    HIP_TRY(hipEventRecord(c->fq_evs[c->job.fq_nev + 1], c->stream));
    c->job.fq_nev += 2;
    c->job.fq_launched = true;
    return FK_OK;
}

// The caller's bytes src[0, off) of this fk_ingest call have landed behind the `have` bytes of
// earlier calls: moves the frontier to the start of the last record not yet known to be complete
// (the input's end with final_), queues the normalisation up to it, and returns it in *limit --
// the map may read below it.  The host looks at the last few lines before have + off only.
static int fq_advance(fk_ctx *c, const uint8_t *src, uint64_t have, uint64_t off, bool final_, uint64_t *limit) {
    const uint64_t end = have + off;
    uint64_t f = end;
    if (!final_) {
        const uint64_t tb = have - c->job.fq_tail.size();  // fq_tail holds [tb, have), tb <= fq_done
        const std::vector<uint8_t> &tail = c->job.fq_tail;
        // at most FQ_LOOK bytes back: a record longer than that moves the frontier once the next one is seen
        constexpr uint64_t FQ_LOOK = 16ull << 20;
        f = fastq_frontier_scan([&](uint64_t p) { return p < have ? tail[p - tb] : src[p - have]; }, c->job.fq_done, end,
                                end > FQ_LOOK ? end - FQ_LOOK : 0);
        if (f == end) f = c->job.fq_done;  // no record start in sight (a long read): the frontier stays
    }
    FK_TRY(fq_normalise(c, nullptr, c->job.fq_done, f, final_));
    c->job.fq_done = f;
    *limit = f;
    return FK_OK;
}

// fk_map / fk_signature_counts: what no fk_ingest(..., last = 1) has normalised ends the input.
static int fq_finish_pending(fk_ctx *c, uint64_t n) {
    if (!c->job.fq_job || c->job.fq_done >= n) return FK_OK;
    FK_TRY(fq_normalise(c, nullptr, c->job.fq_done, n, true));
    c->job.fq_done = n;
    c->job.fq_tail.clear();
    return FK_OK;
}

// Queues the read-back of the job's FASTQ counters behind the normalise launches (the caller's next
// wait on the map stream covers it) / reads them: FK_E_INVALID for a malformed record.
static int fq_info_queue(fk_ctx *c) {
    if (c->job.fq_job && c->job.fq_launched)
        HIP_TRY(hipMemcpyAsync(c->fq_pin.p, c->fq_info.p, 32, hipMemcpyDeviceToHost, c->stream));
    return FK_OK;
}
static int fq_info_read(fk_ctx *c) {
    if (!c->job.fq_job) return FK_OK;
    const uint64_t *h = c->fq_pin.as<uint64_t>();
    const bool any = c->job.fq_launched;
    c->fq_out[0] = any ? h[0] : 0;
    c->fq_out[1] = any ? h[1] : 0;
    c->fq_out[2] = any && h[2] ? ~h[2] : UINT64_MAX;
    c->fq_have_info = true;
    if (any && h[3])
        return set_err(FK_E_INVALID, "FASTQ: more than one line per 4 bytes over a range of the input (the line index overflowed)");
    if (c->fq_out[2] != UINT64_MAX)
        return set_err(FK_E_INVALID, "FASTQ record %llu is malformed (no '@' or '+' line, quality and sequence of "
                                     "different lengths, or the input ends inside it)", (unsigned long long)c->fq_out[2]);
    return FK_OK;
}

static bool premap_eligible(const fk_ctx *c) {
    return c->fused && map_fused_supported(c->cfg.k, c->cfg.m, (uint32_t)c->Bc);
}

// Streamed map: launches the fused map over the tiles whose bytes (and halo)
// lie below `landed`; `final_` = the input ends at `landed` (every remaining
// tile, the last one sets the record total).  Runs on the map stream after
// the copy stream's segment event.
// The map of tiles [t0, t0 + nt) of the input fa[0, n): parse then signature passes in two kernels
// per MAP_VSLOT_TILES tiles (the parse's waves are latency-bound, the passes' VALU-bound; apart, each
// kernel's waves keep the SIMDs busy), or the fused kernel (FASTKMER_SPLIT_MAP=0, the 256-thread
// tiles, probes).  map_vslots is sized by the callers (map_vslots_reserve).
constexpr uint64_t MAP_VSLOT_TILES = 32768;  // ~1.07 GB of FASTA per split launch pair (140 MB of slots)
static int map_vslots_reserve(fk_ctx *c, uint64_t ntiles) {
    if (!map_split(c)) return FK_OK;
    return ensure(c->map_vslots, std::min(ntiles, MAP_VSLOT_TILES) * map_fused_vslot() * 4);
}
static int map_launch(fk_ctx *c, const uint8_t *fa, uint64_t n, int more, uint64_t t0, uint64_t nt, hipStream_t s) {
    const uint64_t cap = map_split(c) ? c->map_vslots.bytes / ((uint64_t)map_fused_vslot() * 4) : 0;
    for (uint64_t b = 0; b < nt;) {
        const uint64_t m = cap ? std::min(cap, nt - b) : nt - b;
        HIP_TRY(launch_map_fused(FUSED_NT, c->cfg.k, c->cfg.m, fa, n, more, t0 + b, m, c->fm,
                                 c->rec_hdr.as<uint32_t>(), c->rec_pos.as<uint16_t>(), c->rec_code.as<uint32_t>(),
                                 c->tcnt.as<uint32_t>(), c->tstat.as<uint32_t>(), c->counters.as<unsigned long long>(),
                                 s, fused_probe(c), cap ? c->map_vslots.as<uint32_t>() : nullptr));
        b += m;
    }
    return FK_OK;
}

static int premap_launch(fk_ctx *c, uint64_t landed, bool final_) {
    const uint64_t tile = fm_tile_bytes(FUSED_NT), span = fm_span_bytes(FUSED_NT);
    const uint64_t end = final_ ? (landed + tile - 1) / tile : (landed >= span ? (landed - span) / tile + 1 : 0);
    if (end <= c->job.pm_tiles) return FK_OK;
    if (c->tcnt.bytes < end * 4 || c->tstat.bytes < end * 8 || c->rec_hdr.bytes < end * map_fused_tcap() * 4 ||
        c->rec_pos.bytes < end * map_fused_tcap() * 2 || c->rec_code.bytes < end * map_fused_cslot() * 4)
        return set_err(FK_E_STATE, "streamed map: %llu tiles exceed the reserved record slots",
                       (unsigned long long)end);
    hipStream_t s = c->stream;
    if (c->job.pm_tiles == 0) HIP_TRY(hipEventRecord(c->ev[10], s));
    FK_TRY(map_launch(c, c->d_fasta, landed, final_ ? 0 : 1, c->job.pm_tiles, end - c->job.pm_tiles, s));
    c->job.pm_tiles = end;
    if (final_) HIP_TRY(hipEventRecord(c->ev[11], s));
    return FK_OK;
}

static int xch_maybe_piece(fk_ctx *c);
static int local_maybe_piece(fk_ctx *c, uint64_t tiles, hipEvent_t mapped);

// Appends host bytes to the device input on the copy stream, in segments.
// Pinned sources are copied by DMA directly; pageable ones through two
// pinned staging buffers (the memcpy of one overlapping the DMA of the
// other).  With the fused map (k_map_fused) every tile whose bytes have
// landed is mapped on the map stream while the next segment is in flight,
// so the PCIe transfer hides the parse + signature work.  Returns once the
// source has been read (the caller's buffer is free); the map of the last
// segment may still be running.
static int comm_fail(fk_ctx *c, int rc);
static int note_held(fk_ctx *c, int rc);

static int ingest_impl(fk_ctx *c, const uint8_t *fasta, size_t n, int last) {
    if (!fasta && n) return set_err(FK_E_INVALID, "null argument");
    DeviceGuard dg_(c->device);
    if (c->d_fasta && c->d_fasta != c->fasta_own.as<uint8_t>()) {
        // a borrowed device input (fk_ingest_device): host chunks cannot be appended
        // to it, but a host ingest that starts a new job replaces it
        if (c->job.dev_open) return set_err(FK_E_STATE, "fk_ingest appending to an fk_ingest_device input");
        c->d_fasta = nullptr;
    }
    hipStream_t s = c->stream, cs = c->copy_stream;
    const bool fresh = c->ingest_fresh || !c->d_fasta;
    if (fresh) {
        c->n_fasta = 0;
        c->ingest_fresh = false;
        if (c->comm) {
            if (c->job.xch.open) return set_err(FK_E_STATE, "fk_ingest: the previous job's exchange is unfinished (fk_finish)");
            FK_TRY(comm_sync(c, c->comm_stream));
        }
        FK_TRY(comm_sync(c, c->xstage));
        HIP_TRY(hipStreamSynchronize(c->tier_side));  // (the heavy tiers of a count that failed half way)
        HIP_TRY(hipStreamSynchronize(s));  // a previous job's work may still read the buffers
        FK_TRY(begin_job(c, c->in_format == FK_FORMAT_FASTQ));
        c->job.pm_active = premap_eligible(c);
    } else if (c->job.pm_last_seen) {
        c->job.pm_active = false;  // appending after the final tiles: fk_map maps the whole input
    }
    const uint64_t have = c->n_fasta, need = have + n;
    if (c->fasta_own.bytes < need) {  // grow, keeping what was ingested (and what the map reads)
        HIP_TRY(hipStreamSynchronize(cs));
        FK_TRY(grow_keep(c->fasta_own, need, have, s));
    }
    c->d_fasta = c->fasta_own.as<uint8_t>();
    // FASTQ: every segment is normalised up to the frontier before the map may read it; the map's
    // limit is the frontier where it is `landed` for FASTA
    const bool fq = c->job.fq_job;
    if (fq) FK_TRY(ensure(c->fq_ws, fastq_ws_bytes(std::min<uint64_t>(n, 4 * c->ingest_seg) + (1u << 20))));
    if (c->job.pm_active) {
        // record slots and per-tile counts of every tile this input can hold (kept on growth)
        const uint64_t tiles = (need + fm_tile_bytes(FUSED_NT) - 1) / fm_tile_bytes(FUSED_NT) + 1;
        if (c->tcnt.bytes < tiles * 4) FK_TRY(grow_keep(c->tcnt, tiles * 4, c->tcnt.bytes, s));
        if (c->tstat.bytes < tiles * 8) FK_TRY(grow_keep(c->tstat, tiles * 8, c->tstat.bytes, s));
        const uint64_t hdr_need = tiles * map_fused_tcap() * 4, pos_need = tiles * map_fused_tcap() * 2;
        const uint64_t code_need = tiles * map_fused_cslot() * 4;
        if (c->rec_hdr.bytes < hdr_need) FK_TRY(grow_keep(c->rec_hdr, hdr_need, c->rec_hdr.bytes, s));
        if (c->rec_pos.bytes < pos_need) FK_TRY(grow_keep(c->rec_pos, pos_need, c->rec_pos.bytes, s));
        if (c->rec_code.bytes < code_need) FK_TRY(grow_keep(c->rec_code, code_need, c->rec_code.bytes, s));
        FK_TRY(map_vslots_reserve(c, tiles));
        if (fresh) {
            FK_TRY(ensure(c->counters, 64));
            HIP_TRY(hipMemsetAsync(c->counters.p, 0, 64, s));
        }
    }
    uint8_t *dst = c->fasta_own.as<uint8_t>() + have;
    hipPointerAttribute_t attr{};
    const bool pinned = hipPointerGetAttributes(&attr, fasta) == hipSuccess && attr.type == hipMemoryTypeHost;
    (void)hipGetLastError();
    if (!pinned && n)
        for (int i = 0; i < 2; ++i)
            if (!c->pinned[i].p) {
                HIP_TRY(c->pinned[i].alloc(PIN_CHUNK, hipHostMallocDefault));
                HIP_TRY(c->pin_ev[i].create(hipEventDisableTiming));
                HIP_TRY(hipEventRecord(c->pin_ev[i], cs));
            }
    // with a communicator, every piece of mapped tiles is exchanged while later ones land
    const bool pieces = c->comm && c->job.pm_active;
    // the job's size: this call's when it holds the whole input, else what fk_ingest_reserve announced
    if (pieces && fresh) {
        c->job.xch.expect_bytes = last ? n : c->reserve_bytes;
        // a job of known size goes out in about XCH_STEPS steps (at most 1 GB, at least XCH_MIN each):
        // every step but the last moves while later bytes are copied in (one 1 GB step for a 1 GB job
        // would leave the whole exchange after the last byte), and the staging cuts (st_cuts) fall on
        // step ends (1 GB steps of a 6.25 GB job staged 5-6 GB after the last byte: 11 ms of expansion
        // in the tail, profiles/r05d_xch1_c3_tail.txt)
        constexpr uint64_t XCH_STEPS = 10;
        constexpr uint64_t XCH_MIN = 64ull << 20;  // a 1 GB job: ten steps (128 MB: seven)
        if (!c->piece_bytes_set)
            c->piece_bytes = c->job.xch.expect_bytes
                                 ? std::min<uint64_t>(1ull << 30, std::max<uint64_t>(XCH_MIN, c->job.xch.expect_bytes / XCH_STEPS))
                                 : 1ull << 30;
    }
    if (fresh) {
        c->job.job_bytes = last ? n : c->reserve_bytes;
        c->reserve_bytes = 0;
    }
    HIP_TRY(hipEventRecord(c->h2d_ev[0], cs));
    if (pinned) {
        // every segment's copy is queued first, so the DMA runs back to back even while the
        // host waits on a piece's exchange.  Each copy boundary costs ~11 us of link time
        // (profiles/r05s_h2d_rates.txt): up to the call's last tenth (at least four small
        // segments) the segments grow to a sixteenth of the call in whole ingest_segs, at most four
        // (1 GB: 64 MB, 6.25 GB: 128 MB; configs[1] 22.70 -> 22.56 ms, profiles/r05z_xch_cuts_seg_ab.txt),
        // with a communicator at most a quarter of an exchange step; ingest_seg in that last tenth, so
        // that what follows the last byte (the last segment's map, the last piece) stays short
        const size_t seg = c->ingest_seg;
        size_t big = seg * std::clamp<size_t>((n / 16 + seg / 2) / seg, 1, 4);
        if (pieces) big = std::min(big, std::max(seg, (size_t)c->piece_bytes / 4 / seg * seg));
        const size_t nseg = (n + seg - 1) / seg;
        const size_t small_from = n - std::min(n, std::max<size_t>(n / 10, 4 * seg));
        auto seg_len = [&](size_t off) { return std::min(off < small_from ? big : seg, n - off); };
        if (c->job.pm_active || fq) HIP_TRY(ensure_events(c->seg_evs, nseg, hipEventDisableTiming));
        size_t off = 0;
        for (size_t i = 0; off < n; ++i) {
            const size_t len = seg_len(off);
            HIP_TRY(hipMemcpyAsync(dst + off, fasta + off, len, hipMemcpyHostToDevice, cs));
            if (c->job.pm_active || fq) HIP_TRY(hipEventRecord(c->seg_evs[i], cs));
            off += len;
        }
        HIP_TRY(hipEventRecord(c->h2d_ev[1], cs));
        // every segment's map is queued too (one rank; the exchange steps wait on the host between
        // them), then the pieces are staged on the staging stream behind the map of their last
        // segment: the host's waits for a piece's partition never hold back a later map launch
        if (!pieces && c->job.pm_active) HIP_TRY(ensure_events(c->map_evs, nseg, hipEventDisableTiming));
        c->seg_tiles.clear();
        off = 0;
        for (size_t i = 0; (c->job.pm_active || fq) && off < n; ++i) {
            off += seg_len(off);
            HIP_TRY(hipStreamWaitEvent(s, c->seg_evs[i], 0));
            uint64_t limit = have + off;
            if (fq) FK_TRY(fq_advance(c, fasta, have, off, last && off == n, &limit));
            if (!c->job.pm_active) continue;
            FK_TRY(premap_launch(c, limit, last && off == n));
            if (pieces) {
                FK_TRY(xch_maybe_piece(c));
            } else {
                HIP_TRY(hipEventRecord(c->map_evs[i], s));
                c->seg_tiles.push_back(c->job.pm_tiles);
            }
        }
        for (size_t i = 0; !pieces && c->job.pm_active && i < c->seg_tiles.size(); ++i)
            FK_TRY(local_maybe_piece(c, c->seg_tiles[i], c->map_evs[i]));
    } else {
        size_t off = 0;
        for (int i = 0; off < n; ++i) {
            const size_t len = std::min(PIN_CHUNK, n - off);
            HIP_TRY(hipEventSynchronize(c->pin_ev[i & 1]));  // its previous DMA is done
            memcpy(c->pinned[i & 1].p, fasta + off, len);
            HIP_TRY(hipMemcpyAsync(dst + off, c->pinned[i & 1].p, len, hipMemcpyHostToDevice, cs));
            HIP_TRY(hipEventRecord(c->pin_ev[i & 1], cs));
            off += len;
            if (c->job.pm_active || fq) {
                HIP_TRY(hipEventRecord(c->seg_ev, cs));
                HIP_TRY(hipStreamWaitEvent(s, c->seg_ev, 0));
                uint64_t limit = have + off;
                if (fq) FK_TRY(fq_advance(c, fasta, have, off, last && off == n, &limit));
                if (!c->job.pm_active) continue;
                FK_TRY(premap_launch(c, limit, last && off == n));
                if (pieces) {
                    FK_TRY(xch_maybe_piece(c));
                } else {
                    HIP_TRY(hipEventRecord(c->seg_ev, s));  // reused: the staging stream waits on it at once
                    FK_TRY(local_maybe_piece(c, c->job.pm_tiles, c->seg_ev));
                }
            }
        }
        HIP_TRY(hipEventRecord(c->h2d_ev[1], cs));
    }
    if (fq) {
        uint64_t limit = 0;
        if (last && n == 0) FK_TRY(fq_advance(c, fasta, have, 0, true, &limit));  // the input ends here
        // the caller's bytes behind the frontier, for the next call's look at the record they begin
        const uint64_t tb = have - c->job.fq_tail.size();
        std::vector<uint8_t> tail;
        if (c->job.fq_done < have) tail.assign(c->job.fq_tail.begin() + (c->job.fq_done - tb), c->job.fq_tail.end());
        const uint64_t from = c->job.fq_done > have ? c->job.fq_done - have : 0;
        if (from < n) tail.insert(tail.end(), fasta + from, fasta + n);
        c->job.fq_tail.swap(tail);
    }
    if (c->job.pm_active && last) {
        c->job.pm_last_seen = true;
        if (n == 0) FK_TRY(premap_launch(c, need, true));
    }
    HIP_TRY(hipStreamSynchronize(cs));  // the source has been read
    c->ms_h2d = ev_ms(c->h2d_ev[0], c->h2d_ev[1]);
    c->n_fasta = need;
    reset_results(c);  // an appending call too
    return FK_OK;
}

// fk_ingest is collective with a communicator (pieces are exchanged while the input lands): any
// error on this rank aborts the group, so peers blocked in a step return instead of waiting.
FK_EXPORT int fk_ingest(fk_ctx *c, const uint8_t *fasta, size_t n, int last) {
    if (!c) return set_err(FK_E_INVALID, "null ctx");
    const int rc = ingest_impl(c, fasta, n, last);
    return rc && c->comm ? comm_fail(c, rc) : note_held(c, rc);
}

static int reserve_impl(fk_ctx *c, uint64_t total_bytes);

FK_EXPORT int fk_ingest_reserve(fk_ctx *c, uint64_t total_bytes) {
    if (!c) return set_err(FK_E_INVALID, "null ctx");
    return reserve_impl(c, total_bytes);
}

static int reserve_impl(fk_ctx *c, uint64_t total_bytes) {
    DeviceGuard dg_(c->device);
    if (!c->ingest_fresh && c->d_fasta) return set_err(FK_E_STATE, "fk_ingest_reserve inside a streamed input");
    FK_TRY(ensure(c->fasta_own, total_bytes));
    c->reserve_bytes = total_bytes;  // the next (streamed) job's size: piece cuts and staged plans follow it
    if (premap_eligible(c)) {
        const uint64_t tiles = (total_bytes + fm_tile_bytes(FUSED_NT) - 1) / fm_tile_bytes(FUSED_NT) + 1;
        FK_TRY(ensure(c->rec_hdr, tiles * map_fused_tcap() * 4));
        FK_TRY(ensure(c->rec_pos, tiles * map_fused_tcap() * 2));
        FK_TRY(ensure(c->rec_code, tiles * map_fused_cslot() * 4));
        FK_TRY(ensure(c->tcnt, tiles * 4));
        FK_TRY(ensure(c->tstat, tiles * 8));
    }
    return FK_OK;
}

// ---- a rank's split of a FASTA file (fk_split.cpp)

namespace {
struct Fd {
    int fd = -1;
    ~Fd() {
        if (fd >= 0) close(fd);
    }
};
int open_split(const char *path, int32_t world, int32_t rank, int32_t k, int32_t seq, Fd &f, uint64_t &size,
               SplitPlan &plan, bool fastq = false) {
    f.fd = open(path, O_RDONLY | O_CLOEXEC);
    if (f.fd < 0) return set_err(FK_E_IO, "open(%s): %s", path, strerror(errno));
    struct stat st {};
    if (fstat(f.fd, &st) != 0) return set_err(FK_E_IO, "fstat(%s): %s", path, strerror(errno));
    size = (uint64_t)st.st_size;
    std::string err;
    if (seq != 0 && seq != 1) return set_err(FK_E_INVALID, "sequence_type must be 0 or 1");
    if (fastq ? plan_split_fastq(f.fd, size, world, rank, plan, err) : plan_split(f.fd, size, world, rank, k, seq, plan, err))
        return set_err(world < 1 || rank < 0 || rank >= world || k < 1 ? FK_E_INVALID : FK_E_IO, "%s: %s", path,
                       err.c_str());
    return FK_OK;
}
}  // namespace

FK_EXPORT int fk_split_bytes(const char *path, int32_t world, int32_t rank, int32_t k, int32_t sequence_type,
                             uint8_t *out, size_t cap, size_t *n) {
    if (!path || !n) return set_err(FK_E_INVALID, "null argument");
    Fd f;
    uint64_t size = 0;
    SplitPlan plan;
    FK_TRY(open_split(path, world, rank, k, sequence_type, f, size, plan));
    *n = (size_t)plan.total;
    if (!out) return FK_OK;
    if (cap < plan.total) return set_err(FK_E_RANGE, "split of %llu bytes, buffer holds %zu", (unsigned long long)plan.total, cap);
    std::string err;
    if (read_split(f.fd, size, plan, 0, plan.total, out, err)) return set_err(FK_E_IO, "%s: %s", path, err.c_str());
    return FK_OK;
}

FK_EXPORT int fk_split_bytes_fastq(const char *path, int32_t world, int32_t rank, uint8_t *out, size_t cap, size_t *n) {
    if (!path || !n) return set_err(FK_E_INVALID, "null argument");
    Fd f;
    uint64_t size = 0;
    SplitPlan plan;
    FK_TRY(open_split(path, world, rank, 1, 0, f, size, plan, true));
    *n = (size_t)plan.total;
    if (!out) return FK_OK;
    if (cap < plan.total) return set_err(FK_E_RANGE, "split of %llu bytes, buffer holds %zu", (unsigned long long)plan.total, cap);
    std::string err;
    if (read_split(f.fd, size, plan, 0, plan.total, out, err)) return set_err(FK_E_IO, "%s: %s", path, err.c_str());
    return FK_OK;
}

// With a communicator the split is the job's: (world, rank) must be the context's own (a mismatch
// would count some byte ranges twice and skip others while the exchange still completes).
static int check_split_rank(const fk_ctx *c, int32_t world, int32_t rank, const char *what) {
    if (c->comm && (world != (int32_t)c->G || rank != c->cfg.rank))
        return set_err(FK_E_INVALID, "%s: split %d of %d on the context of rank %d of %u", what, rank, world,
                       c->cfg.rank, c->G);
    return FK_OK;
}

static int ingest_file_impl(fk_ctx *c, const char *path, int32_t world, int32_t rank, uint64_t window) {
    if (!path) return set_err(FK_E_INVALID, "null path");
    FK_TRY(check_split_rank(c, world, rank, "fk_ingest_file_range"));
    if (!c->ingest_fresh && c->d_fasta) return set_err(FK_E_STATE, "fk_ingest_file_range inside a streamed input");
    Fd f;
    uint64_t size = 0;
    SplitPlan plan;
    FK_TRY(open_split(path, world, rank, c->cfg.k, c->cfg.sequence_type, f, size, plan, c->in_format == FK_FORMAT_FASTQ));
    const uint64_t total = plan.total;
    if (total == 0) return ingest_impl(c, nullptr, 0, 1);
    if (!window) window = 256ull << 20;
    window = std::max<uint64_t>(window, 1ull << 20);
    const uint64_t win = std::min(window, total);
    for (int i = 0; i < 2 && i * win < total; ++i)
        if (c->file_pin[i].ensure(win)) return set_err(FK_E_NOMEM, "hipHostMalloc(%llu) failed", (unsigned long long)win);
    FK_TRY(reserve_impl(c, total));
    std::string rerr;
    int rrc = read_split(f.fd, size, plan, 0, win, c->file_pin[0].as<uint8_t>(), rerr);
    if (rrc) return set_err(FK_E_IO, "%s: %s", path, rerr.c_str());
    int b = 0;
    for (uint64_t pos = 0; pos < total;) {
        const uint64_t len = std::min(win, total - pos), next = std::min(win, total - pos - len);
        // the next window is read while this one is copied and mapped
        std::thread reader;
        if (next)
            reader = std::thread([&, b, pos, len, next] {
                rrc = read_split(f.fd, size, plan, pos + len, next, c->file_pin[b ^ 1].as<uint8_t>(), rerr);
            });
        const int rc = ingest_impl(c, c->file_pin[b].as<uint8_t>(), len, pos + len == total ? 1 : 0);
        if (reader.joinable()) reader.join();
        if (rc) return rc;
        if (rrc) return set_err(FK_E_IO, "%s: %s", path, rerr.c_str());
        pos += len;
        b ^= 1;
    }
    return FK_OK;
}

FK_EXPORT int fk_ingest_file_range(fk_ctx *c, const char *path, int32_t world, int32_t rank, uint64_t window_bytes) {
    if (!c) return set_err(FK_E_INVALID, "null ctx");
    const int rc = ingest_file_impl(c, path, world, rank, window_bytes);
    return rc && c->comm ? comm_fail(c, rc) : rc;
}

static int ingest_device_impl(fk_ctx *c, const void *d, size_t n, int last);

FK_EXPORT int fk_ingest_device(fk_ctx *c, const void *d, size_t n, int last) {
    if (!c) return set_err(FK_E_INVALID, "null ctx");
    const int rc = ingest_device_impl(c, d, n, last);
    return rc && c->comm ? comm_fail(c, rc) : rc;
}

static int ingest_device_impl(fk_ctx *c, const void *d, size_t n, int last) {
    if (!d && n) return set_err(FK_E_INVALID, "null argument");
    DeviceGuard dg_(c->device);
    if (c->comm && c->job.xch.open) return set_err(FK_E_STATE, "fk_ingest_device: the previous job's exchange is unfinished");
    c->ingest_fresh = true;
    FK_TRY(begin_job(c, c->in_format == FK_FORMAT_FASTQ));
    c->job.dev_open = last == 0;  // a borrowed input takes no appended host chunks
    if (c->job.fq_job) {
        // the borrowed buffer stays as it is: the stage copies it into fasta_own as it reads it
        FK_TRY(ensure(c->fasta_own, n));
        FK_TRY(fq_normalise(c, (const uint8_t *)d, 0, n, true));
        c->job.fq_done = n;
        c->d_fasta = c->fasta_own.as<uint8_t>();
    } else if (((uintptr_t)d & 15) != 0) {
        FK_TRY(ensure(c->fasta_own, n));
        HIP_TRY(hipMemcpyAsync(c->fasta_own.p, d, n, hipMemcpyDeviceToDevice, c->stream));
        c->d_fasta = c->fasta_own.as<uint8_t>();
    } else {
        c->d_fasta = (const uint8_t *)d;
    }
    c->n_fasta = n;
    return FK_OK;
}

FK_EXPORT int fk_synth_fasta_to_device(void *d_out, uint64_t first_read, uint64_t n_reads, int32_t read_len,
                                       uint64_t genome_len, uint64_t seed, double err_rate, double n_rate) {
    if ((!d_out && n_reads) || read_len < 1 || genome_len < 1) return set_err(FK_E_INVALID, "bad synth arguments");
    const SynthParams p = make_synth(first_read, n_reads, read_len, genome_len, seed, err_rate, n_rate);
    const uint64_t nb = n_reads * p.rec_bytes;
    if (nb) HIP_TRY(launch_synth((uint8_t *)d_out, nb, p, nullptr));
    HIP_TRY(hipDeviceSynchronize());
    return FK_OK;
}

FK_EXPORT int fk_synth_fasta_device(fk_ctx *c, uint64_t first_read, uint64_t n_reads, int32_t read_len,
                                    uint64_t genome_len, uint64_t seed, double err_rate, double n_rate) {
    if (!c || read_len < 1 || genome_len < 1) return set_err(FK_E_INVALID, "bad synth arguments");
    DeviceGuard dg_(c->device);
    const SynthParams p = make_synth(first_read, n_reads, read_len, genome_len, seed, err_rate, n_rate);
    const uint64_t nb = n_reads * p.rec_bytes;
    FK_TRY(ensure(c->fasta_own, nb));
    if (c->comm && c->job.xch.open) return set_err(FK_E_STATE, "fk_synth_fasta_device: the previous job's exchange is unfinished");
    HIP_TRY(launch_synth(c->fasta_own.as<uint8_t>(), nb, p, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->ingest_fresh = true;
    FK_TRY(begin_job(c, false));  // synthetic FASTA, whatever the context's format
    c->d_fasta = c->fasta_own.as<uint8_t>();
    c->n_fasta = nb;
    return FK_OK;
}

// ---------------------------------------------------------------------------
// map side: parse + encode + signature + records (+ destination histogram)
// ---------------------------------------------------------------------------


// Fused parse + signature (k_map_fused): FASTA bytes to records in one kernel.
// *ok = false when a tile raised the fallback flag (the caller then maps with
// the two-kernel path, which places every input).
static int map_fused(fk_ctx *c, uint64_t n, bool *ok) {
    hipStream_t s = c->stream;
    *ok = false;
    const uint64_t tile = fm_tile_bytes(FUSED_NT);
    const uint64_t ntiles = (n + tile - 1) / tile;
    FK_TRY(ensure(c->tcnt, ntiles * 4));
    FK_TRY(ensure(c->tstat, ntiles * 8));
    FK_TRY(ensure(c->counters, 64));
    FK_TRY(ensure(c->rec_hdr, ntiles * map_fused_tcap() * 4));
    FK_TRY(ensure(c->rec_pos, ntiles * map_fused_tcap() * 2));
    FK_TRY(ensure(c->rec_code, ntiles * map_fused_cslot() * 4));
    FK_TRY(map_vslots_reserve(c, ntiles));
    HIP_TRY(hipEventRecord(c->ev[2], s));
    HIP_TRY(hipMemsetAsync(c->counters.p, 0, 64, s));
    HIP_TRY(hipEventRecord(c->ev[10], s));
    FK_TRY(map_launch(c, c->d_fasta, n, 0, 0, ntiles, s));
    HIP_TRY(hipEventRecord(c->ev[11], s));
    HIP_TRY(launch_tile_totals(c->tcnt.as<uint32_t>(), c->tstat.as<uint32_t>(), ntiles,
                               c->counters.as<unsigned long long>(), s));
    HIP_TRY(hipEventRecord(c->ev[3], s));
    uint64_t h[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(h, c->counters.p, 32, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    c->stats.fused_fallback = h[2];
    if (h[2]) return FK_OK;  // fallback
    c->nrec = h[0];
    c->nkmers = h[1];
    c->stats.positions = h[3];
    c->rec_tiled = true;
    c->rec_tiles = ntiles;
    *ok = true;
    c->stats.ms_parse = 0.0;
    c->stats.ms_signature = ev_ms(c->ev[2], c->ev[3]);
    c->stats.ms_encode_kernel = 0.0;
    c->stats.ms_signature_kernel = ev_ms(c->ev[10], c->ev[11]);
    return FK_OK;
}

// the fused map's tiles [t0, t0 + nt) as a partition source (nrec: their records, or a bound)
static RecSrc fused_src(const fk_ctx *c, uint64_t t0, uint64_t nt, uint64_t nrec) {
    const uint64_t tcap = map_fused_tcap(), cslot = map_fused_cslot();
    return tiled_src(c->rec_hdr.as<uint32_t>() + t0 * tcap, c->rec_pos.as<uint16_t>() + t0 * tcap,
                     c->rec_code.as<uint32_t>() + t0 * cslot, c->tcnt.as<uint32_t>() + t0, nrec, nt, (uint32_t)tcap,
                     (uint32_t)cslot, c->W, c->cfg.k);
}

// the records of the last fk_map as a partition source
static RecSrc map_src(const fk_ctx *c) {
    if (c->rec_tiled) return fused_src(c, 0, c->rec_tiles, c->nrec);
    return dense_src(c->records.as<uint64_t>(), c->nrec, c->W);
}

// fk_map steps 0-2: the input's super-k-mer records (fused kernel, or parse + signature)
static int map_records(fk_ctx *c) {
    const double t_start = now_ms();
    hipStream_t s = c->stream;
    c->ingest_fresh = true;  // a later fk_ingest starts a new input
    c->job.dev_open = false;
    const uint64_t n = c->d_fasta ? c->n_fasta : 0;
    new_result(c);
    c->stats.fasta_bytes = n;
    c->job.job_open = false;
    // FASTQ: what is left behind the frontier ends the input; the stage's counters and its malformed
    // flag come back with the map's own read-back below (every path with input waits on the stream)
    FK_TRY(fq_finish_pending(c, n));
    FK_TRY(fq_info_queue(c));

    // 0. fused parse + signature (streamed by fk_ingest, or one launch here); the
    // two-kernel path below maps the inputs the fused kernel hands back
    bool fused_ok = false;
    c->stats.ms_h2d = c->ms_h2d;
    if (c->job.pm_active && n) {
        // streamed map (fk_ingest launched the tiles as their bytes landed)
        if (!c->job.pm_last_seen) FK_TRY(premap_launch(c, n, true));  // the input ends here
        HIP_TRY(launch_tile_totals(c->tcnt.as<uint32_t>(), c->tstat.as<uint32_t>(), c->job.pm_tiles,
                                   c->counters.as<unsigned long long>(), s));
        uint64_t h[4] = {0, 0, 0, 0};
        HIP_TRY(hipMemcpyAsync(h, c->counters.p, 32, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        c->stats.fused_fallback = h[2];
        if (!h[2]) {
            fused_ok = true;
            c->rec_tiled = true;
            c->rec_tiles = c->job.pm_tiles;
            c->nrec = h[0];
            c->nkmers = h[1];
            c->stats.positions = h[3];
            c->stats.ms_parse = 0.0;
            // map stream from the first to the last launch, waits for the landing segments included
            c->stats.ms_signature = ev_ms(c->ev[10], c->ev[11]);
            c->stats.ms_signature_kernel = c->stats.ms_signature;
        }
        c->job.pm_active = false;
    } else if (c->fused && n && map_fused_supported(c->cfg.k, c->cfg.m, (uint32_t)c->Bc)) {
        FK_TRY(map_fused(c, n, &fused_ok));
    }
    c->job.pm_active = false;

    const uint64_t ntiles = (n + ENC_TILE - 1) / ENC_TILE;
    const uint64_t code_words = n / 16 + 2 * POS_PAD_WORDS + 512;
    const uint64_t valid_words = n / 32 + 2 * POS_PAD_WORDS + 512;
    const uint64_t sig_tiles = (n + SIG_TILE - 1) / SIG_TILE + 1;
    if (!fused_ok) {
        FK_TRY(ensure(c->tile_last_nl, ntiles * 8));  // look-back status: newline / header state
        FK_TRY(ensure(c->tile_off, ntiles * 8));      // look-back status: output positions
        FK_TRY(ensure(c->npos_dev, 16));  // [0] positions, [1] "rerun the parse with the look-back"
        FK_TRY(ensure(c->codes, code_words * 4));
        FK_TRY(ensure(c->valid, valid_words * 4));
        FK_TRY(ensure(c->counters, 64));
        FK_TRY(ensure(c->sig_status, sig_tiles * 8));
        FK_TRY(ensure(c->sig_kmers, sig_tiles * 8));
    }

    // 1. FASTA parse + 2-bit encode.  The scan variant flags inputs it cannot
    // place (a line longer than its read-back, text before the first header);
    // the flag is read with the record count below and the parse is redone
    // with the line look-back.
    auto run_parse = [&](bool scan) -> int {
        HIP_TRY(hipEventRecord(c->ev[0], s));
        HIP_TRY(hipMemsetAsync(c->codes.p, 0, code_words * 4, s));
        HIP_TRY(hipMemsetAsync(c->valid.p, 0, valid_words * 4, s));
        HIP_TRY(hipMemsetAsync(c->npos_dev.p, 0, 16, s));
        if (n) {
            if (!scan) HIP_TRY(hipMemsetAsync(c->tile_last_nl.p, 0, ntiles * 8, s));
            HIP_TRY(hipMemsetAsync(c->tile_off.p, 0, ntiles * 8, s));
            HIP_TRY(hipEventRecord(c->ev[8], s));
            HIP_TRY(launch_fasta_parse(scan, c->d_fasta, n, c->tile_last_nl.as<uint64_t>(), c->tile_off.as<uint64_t>(),
                                       c->codes.as<uint32_t>(), c->valid.as<uint32_t>(), c->npos_dev.as<uint64_t>(),
                                       s));
            HIP_TRY(hipEventRecord(c->ev[9], s));
        }
        HIP_TRY(hipEventRecord(c->ev[1], s));
        return FK_OK;
    };
    c->last_map_fused = fused_ok;
    c->stats.fused_map = fused_ok ? 1 : 0;
    bool parse_scan = true;  // the scan variant first; the look-back rerun if it flags the input
    if (!fused_ok) FK_TRY(run_parse(parse_scan));

    // 2. signature + super-k-mer records (retried once if the capacity estimate was short)
    uint64_t rec_cap = std::max<uint64_t>(n / 6, 4096);
    for (int attempt = 0; attempt < 2 && !fused_ok; ++attempt) {
        FK_TRY(ensure(c->records, rec_cap * c->W * 8));
        rec_cap = c->records.bytes / (c->W * 8);
        HIP_TRY(hipMemsetAsync(c->counters.p, 0, 64, s));
        HIP_TRY(hipEventRecord(c->ev[2], s));
        HIP_TRY(hipMemsetAsync(c->sig_status.p, 0, sig_tiles * 8, s));
        HIP_TRY(hipMemsetAsync(c->sig_kmers.p, 0, sig_tiles * 8, s));
        HIP_TRY(hipEventRecord(c->ev[10], s));
        HIP_TRY(launch_superkmers(c->W, c->codes.as<uint32_t>(), c->valid.as<uint32_t>(), n,
                                  c->npos_dev.as<uint64_t>(), c->cfg.k, c->cfg.m, c->fm, c->records.as<uint64_t>(),
                                  rec_cap, c->sig_status.as<uint64_t>(), c->sig_kmers.as<uint64_t>(),
                                  c->counters.as<unsigned long long>(), s));
        HIP_TRY(hipEventRecord(c->ev[11], s));
        // total k-mers = sum of the per-tile counts (into counters[1])
        HIP_TRY(scan_excl_sum_u64(c->sig_kmers.as<uint64_t>(), c->sig_status.as<uint64_t>(), sig_tiles,
                                  c->counters.as<uint64_t>() + 1, c->ws, s));
        HIP_TRY(hipEventRecord(c->ev[3], s));
        uint64_t h[2], redo = 0;
        HIP_TRY(hipMemcpyAsync(h, c->counters.p, 16, hipMemcpyDeviceToHost, s));
        if (parse_scan) HIP_TRY(hipMemcpyAsync(&redo, c->npos_dev.as<uint64_t>() + 1, 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (redo) {
            parse_scan = false;
            FK_TRY(run_parse(false));
            --attempt;
            continue;
        }
        c->nrec = h[0];
        c->nkmers = h[1];
        if (c->nrec <= rec_cap) break;
        rec_cap = c->nrec;
    }
    if (!fused_ok) {
        uint64_t npos = 0;
        HIP_TRY(hipMemcpy(&npos, c->npos_dev.p, 8, hipMemcpyDeviceToHost));
        c->stats.positions = npos;
        c->stats.ms_parse = ev_ms(c->ev[0], c->ev[1]);
        c->stats.ms_signature = ev_ms(c->ev[2], c->ev[3]);
        c->stats.ms_encode_kernel = n ? ev_ms(c->ev[8], c->ev[9]) : 0.0;
        c->stats.ms_signature_kernel = ev_ms(c->ev[10], c->ev[11]);
    }
    c->stats.kmers = c->nkmers;
    c->stats.superkmers = c->nrec;
    c->stats.ms_total += now_ms() - t_start;
    return fq_info_read(c);
}

// Grouped emit: records and k-mers of the mapped records per (destination, local bin) part and the
// send counts per destination, under the current group table (the receiver needs no partition pass).
static int grouped_part_counts(fk_ctx *c) {
    hipStream_t s = c->stream;
    const uint32_t nparts = c->G * c->grp_nlb;
    c->grp_rec.assign(nparts, 0);
    c->grp_kmer.assign(nparts, 0);
    c->send_counts.assign(c->G, 0);
    if (c->nrec) {
        FK_TRY(part_count(c->dest, map_src(c), 0, c->G, c->grp_table.as<uint32_t>(), nparts, c->ws, s));
        HIP_TRY(hipMemcpyAsync(c->grp_rec.data(), c->dest.rec.p, (uint64_t)nparts * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(c->grp_kmer.data(), c->dest.kmer.p, (uint64_t)nparts * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    for (uint32_t d = 0; d < c->G; ++d)
        for (uint32_t lb = 0; lb < c->grp_nlb; ++lb) c->send_counts[d] += c->grp_rec[(uint64_t)d * c->grp_nlb + lb];
    return FK_OK;
}

static int build_group_table(fk_ctx *c);

FK_EXPORT int fk_map(fk_ctx *c, uint64_t *send_counts) {
    if (!c) return set_err(FK_E_INVALID, "null ctx");
    DeviceGuard dg_(c->device);
    // one rank: the pieces staged during fk_ingest read the mapped tiles on the staging stream
    if (c->job.st_np && !c->comm) HIP_TRY(hipStreamWaitEvent(c->stream, c->xstage_ev, 0));
    FK_TRY(map_records(c));
    const double t_start = now_ms();
    hipStream_t s = c->stream;

    // 3a. destination histogram (records per rank)
    c->send_counts.assign(c->G, 0);
    if (c->grouped) {
        FK_TRY(grouped_part_counts(c));
    } else if (c->G == 1) {
        c->send_counts[0] = c->nrec;
    } else if (c->nrec) {
        FK_TRY(part_count(c->dest, map_src(c), 0, c->G, owner_table(c), c->G, c->ws, s));
        HIP_TRY(hipMemcpyAsync(c->send_counts.data(), c->dest.rec.p, c->G * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    if (send_counts)
        for (uint32_t r = 0; r < c->G; ++r) send_counts[r] = c->send_counts[r];
    c->mapped = true;
    c->stats.ms_total += now_ms() - t_start;
    return FK_OK;
}

FK_EXPORT int fk_map_emit(fk_ctx *c, void *d_send, uint64_t cap_records) {
    if (!c) return set_err(FK_E_INVALID, "null ctx");
    DeviceGuard dg_(c->device);
    if (!c->mapped) return set_err(FK_E_STATE, "fk_map_emit before fk_map");
    if (cap_records < c->nrec) return set_err(FK_E_RANGE, "send buffer holds %llu records, need %llu",
                                              (unsigned long long)cap_records, (unsigned long long)c->nrec);
    if (!c->nrec) return FK_OK;
    const double t0 = now_ms();
    hipStream_t s = c->stream;
    if (c->grouped) {
        FK_TRY(part_scatter(c->dest, 0, c->G, c->grp_table.as<uint32_t>(), (uint64_t *)d_send, s));
    } else if (c->G == 1 && !c->rec_tiled) {
        HIP_TRY(hipMemcpyAsync(d_send, c->records.p, c->nrec * c->W * 8, hipMemcpyDeviceToDevice, s));
    } else if (c->G == 1) {  // the fused map's tiles, made dense
        FK_TRY(part_count(c->dest, map_src(c), 0, 1, nullptr, 1, c->ws, s));
        FK_TRY(part_scatter(c->dest, 0, 1, nullptr, (uint64_t *)d_send, s));
    } else {
        FK_TRY(part_scatter(c->dest, 0, c->G, owner_table(c), (uint64_t *)d_send, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    c->stats.ms_total += now_ms() - t0;
    return FK_OK;
}

// ---------------------------------------------------------------------------
// size-aware placement (MultiprocessorSchedulingPartitioner, SBKC:1023-1025)
// ---------------------------------------------------------------------------

FK_EXPORT int fk_map_bin_kmers(fk_ctx *c, uint64_t *kmers_per_bin) {
    if (!c || !kmers_per_bin) return set_err(FK_E_INVALID, "null argument");
    DeviceGuard dg_(c->device);
    if (!c->mapped) return set_err(FK_E_STATE, "fk_map_bin_kmers before fk_map");
    hipStream_t s = c->stream;
    FK_TRY(part_count(c->binhist, map_src(c), 1, 1, nullptr, (uint32_t)c->Bc, c->ws, s));
    HIP_TRY(hipMemcpyAsync(kmers_per_bin, c->binhist.kmer.p, (uint64_t)c->Bc * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return FK_OK;
}

FK_EXPORT int fk_lpt_owners(const uint64_t *sizes, int32_t nbins, int32_t nranks, int32_t *owner) {
    if (!sizes || !owner || nbins < 0 || nranks < 1) return set_err(FK_E_INVALID, "bad argument");
    // largest first onto the least loaded rank (ties: lowest bin, lowest rank); bins of
    // size 0 were not seen by the estimate and keep the hash placement bin % nranks
    std::vector<int32_t> order;
    for (int32_t b = 0; b < nbins; ++b) {
        if (sizes[b])
            order.push_back(b);
        else
            owner[b] = b % nranks;
    }
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return sizes[a] > sizes[b]; });
    std::vector<uint64_t> load(nranks, 0);
    for (int32_t b : order) {
        int32_t r = 0;
        for (int32_t q = 1; q < nranks; ++q)
            if (load[q] < load[r]) r = q;
        owner[b] = r;
        load[r] += sizes[b];
    }
    return FK_OK;
}

FK_EXPORT int fk_set_bin_owners(fk_ctx *c, const int32_t *owner, uint64_t *send_counts) {
    if (!c || !owner) return set_err(FK_E_INVALID, "null argument");
    DeviceGuard dg_(c->device);
    if (c->comm && c->job.xch.open) return set_err(FK_E_STATE, "fk_set_bin_owners inside a job's exchange");
    for (int32_t b = 0; b < c->Bc; ++b)
        if (owner[b] < 0 || (uint32_t)owner[b] >= c->G)
            return set_err(FK_E_INVALID, "owner[%d] = %d is not a rank of %u", b, owner[b], c->G);
    hipStream_t s = c->stream;
    c->h_owner.assign(owner, owner + c->Bc);
    c->h_bin_lbin.assign(c->Bc, ~0u);
    c->h_lbin_bin.clear();
    for (int32_t b = 0; b < c->Bc; ++b)
        if (owner[b] == c->cfg.rank) {
            c->h_bin_lbin[b] = (uint32_t)c->h_lbin_bin.size();
            c->h_lbin_bin.push_back(b);
        }
    c->nlb = (uint32_t)c->h_lbin_bin.size();
    // device maps over every value the 22-bit record bin field can hold
    const uint64_t ntab = (uint64_t)REC_BIN_MASK + 1;
    FK_TRY(ensure(c->d_owner, ntab * 4));
    FK_TRY(ensure(c->d_local, ntab * 4));
    HIP_TRY(hipMemsetAsync(c->d_owner.p, 0xff, ntab * 4, s));
    HIP_TRY(hipMemsetAsync(c->d_local.p, 0xff, ntab * 4, s));
    HIP_TRY(hipMemcpyAsync(c->d_owner.p, c->h_owner.data(), (uint64_t)c->Bc * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(c->d_local.p, c->h_bin_lbin.data(), (uint64_t)c->Bc * 4, hipMemcpyHostToDevice, s));
    c->custom_owners = true;
    c->have_result = false;
    if (c->grouped) {  // the (owner, local bin) parts of the grouped emit follow the new owners
        FK_TRY(build_group_table(c));
        if (c->mapped) FK_TRY(grouped_part_counts(c));  // ... and so do the mapped records' parts
    } else if (c->mapped) {  // the destinations of the mapped records changed
        c->send_counts.assign(c->G, 0);
        if (c->G == 1) {
            c->send_counts[0] = c->nrec;
        } else if (c->nrec) {
            FK_TRY(part_count(c->dest, map_src(c), 0, c->G, owner_table(c), c->G, c->ws, s));
            HIP_TRY(hipMemcpyAsync(c->send_counts.data(), c->dest.rec.p, c->G * 8, hipMemcpyDeviceToHost, s));
        }
    }
    HIP_TRY(hipStreamSynchronize(s));
    if (send_counts)
        for (uint32_t r = 0; r < c->G; ++r) send_counts[r] = c->mapped ? c->send_counts[r] : 0;
    return FK_OK;
}

FK_EXPORT int fk_bin_owners(const fk_ctx *c, int32_t *owner) {
    if (!c || !owner) return set_err(FK_E_INVALID, "null argument");
    for (int32_t b = 0; b < c->Bc; ++b) owner[b] = c->custom_owners ? c->h_owner[b] : (int32_t)((uint32_t)b % c->G);
    return FK_OK;
}

// ---------------------------------------------------------------------------
// reduce side
// ---------------------------------------------------------------------------

// The tiered count, and with it staged pieces (one rank's landed pieces, or the received segments):
// k <= 63 (k = 64 counts the whole input after the last byte, one workgroup per bucket; so do the
// test hook that routes every bucket through the streaming path and the bucket-kernel probes)
static bool staged_ok(const fk_ctx *c) {
#ifdef FK_PROBES
    if (c->dbg_phase != 99) return false;
#endif
    return c->cfg.k <= 63 && !c->force_large;
}

SortedPlan sorted_plan(const fk_ctx *c, uint64_t max_bin_kmers, int force_F) {
    SortedPlan pl;
    const int k = c->cfg.k;
    const uint32_t cap = 2048;  // keys per LDS bucket (k_bucket_count64 / 128-bit k_bucket_sort)
    // cell bits: the largest bin's cells average cap/4 keys (a bucket groups a
    // few cells; runs of one chunk's keys per cell stay long enough to be
    // written as whole lines)
    // (two-level expansion, 64-bit keys: 512 since round 6 -- half the cells of
    // round 2's cap / 8, so the bucket cut and the last piece's level 2 touch
    // half the cell words: configs[2] load 146.9 -> 146.3 ms, configs[1] equal,
    // profiles/r06r_cell_target.txt; 128-bit keys keep 128 per cell)
    // k = 64 (no spare bit in a 128-bit key's hi word): one-level scatter, one workgroup per bucket
    const bool tiered = staged_ok(c);
    const bool two_level = c->cfg.k <= 63;
    constexpr uint64_t CELL_TARGET64 = 512;  // keys per cell of the largest bin, 64-bit keys, two levels
    const uint64_t target = c->cell_target ? c->cell_target
                                           : (c->KW == 2 && tiered ? WAVE128_BUCKET_CAP / 2
                                                                   : two_level ? CELL_TARGET64 : cap / 4);
    int F = 1;
    while (F < MAX_FINE_BITS && ((uint64_t)1 << F) * target < max_bin_kmers) ++F;
    if (!two_level) F = std::min(F, MAX_FINE_BITS - 1);  // one-level scatter: 8 << F bytes of LDS <= 128 KB
    F = std::min(F, 2 * k);
    if (force_F) F = force_F;  // fk_debug_count_pieces: the caller's cells, everything else as the product's
    // k <= 63: two levels (super-cells, then cells; one level measured slower, DESIGN.md §4 "Count" 7);
    // cells per super-cell: 2^5 up to F = 13, 2^6 above (measured at configs[1] and at 8x larger bins)
    const uint32_t wave_cap = c->KW == 1 ? WAVE_BUCKET_CAP : WAVE128_BUCKET_CAP;
    const int F2 = std::min(F, std::max(5, std::min(6, F - 8))), F1 = F - F2;
    pl.F = F, pl.F2 = F2, pl.F1 = F1, pl.tiered = tiered, pl.two_level = two_level, pl.cap = cap, pl.wave_cap = wave_cap;
    pl.max_bin = max_bin_kmers;
    return pl;
}

// 4: expand the records (chunk table at c->chunks, records at c->rsrc) into canonical k-mers laid
// out bin-major by cell in `keys`; c->cell_total = the cell totals, `cell_base` their exclusive
// scan (ncell_all + 1 entries).  Queued on `on`; `cut` (or null): the side stream on which the job's
// bucket cut follows the cell offsets, beside the expansion levels (side_ev[2] tells it)
static int sorted_expand(fk_ctx *c, StreamWs on, hipStream_t cut, const SortedPlan &pl, uint32_t nchunks,
                         uint64_t total_kmers, DevBuf &keys, DevBuf &cell_base_buf) {
    hipStream_t s = on.s;
    const int k = c->cfg.k;
    const int F = pl.F, F2 = pl.F2, F1 = pl.F1;
    const bool two_level = pl.two_level;
    const uint32_t ncell = 1u << F;
    const uint64_t ncell_all = (uint64_t)c->nlb << F;
    FK_TRY(ensure(keys, total_kmers * 8 * c->KW));
    FK_TRY(ensure(c->cell_total, ncell_all * 8));
    FK_TRY(ensure(cell_base_buf, (ncell_all + 1) * 8));
    uint64_t *const cell_base = cell_base_buf.as<uint64_t>();
    // 4: expand records -> canonical k-mers, laid out bin-major by cell
    if (two_level) {
        // cell totals by atomics, per-chunk counts only per super-cell
        const uint64_t nsc_all = (uint64_t)c->nlb << F1;
        FK_TRY(ensure(c->lp, ((uint64_t)nchunks << F1) * 4));
        FK_TRY(ensure(c->sc_total, nsc_all * 8));
        // bins split into pieces of chunks so that ~HIST_PIECES workgroups balance over the CUs (one
        // workgroup per bin waits for the largest bin when bins are few and large)
        constexpr double HIST_PIECES = 1024.0;
        std::vector<uint32_t> pieces, first;
        bool split = false;
        if (nchunks && c->h_bcb.size() == (size_t)c->nlb + 1) {
            for (uint32_t lb = 0; lb < c->nlb; ++lb) {
                const uint32_t cb = c->h_bcb[lb], ce = c->h_bcb[lb + 1], nc = ce - cb;
                const uint32_t P = std::max(1u, std::min(nc, (uint32_t)(HIST_PIECES * nc / nchunks + 0.5)));
                const uint32_t f = (uint32_t)(pieces.size() / 4);
                for (uint32_t q = 0; q < P; ++q) {
                    pieces.insert(pieces.end(), {lb, cb + nc * q / P, cb + nc * (q + 1) / P, P == 1 ? 1u : 0u});
                    first.push_back(f);
                }
                split |= P > 1;
            }
        }
        if (split) {
            const uint32_t np = (uint32_t)first.size();
            FK_TRY(ensure(c->hpieces, (uint64_t)np * 16));
            FK_TRY(ensure(c->hpiece_first, (uint64_t)np * 4));
            FK_TRY(ensure(c->hpiece_tot, ((uint64_t)np << F1) * 4));
            HIP_TRY(hipMemcpyAsync(c->hpieces.p, pieces.data(), (uint64_t)np * 16, hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemcpyAsync(c->hpiece_first.p, first.data(), (uint64_t)np * 4, hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemsetAsync(c->cell_total.p, 0, ncell_all * 8, s));
            HIP_TRY(launch_expand_hist_pieces(c->KW, c->rsrc, c->chunks.as<Chunk>(), c->hpieces.as<uint4>(),
                                              c->hpiece_first.as<uint32_t>(), np, k, F, F2,
                                              c->cell_total.as<uint64_t>(), c->lp.as<uint32_t>(),
                                              c->hpiece_tot.as<uint32_t>(), s));
            HIP_TRY(hipStreamSynchronize(s));  // the host piece tables are released below
        } else {
            HIP_TRY(launch_expand_hist_bin(c->KW, c->rsrc, c->chunks.as<Chunk>(), c->bin_chunk_begin.as<uint32_t>(),
                                           c->nlb, k, F, F2, c->cell_total.as<uint64_t>(), c->lp.as<uint32_t>(), s));
        }
    } else {
        FK_TRY(ensure(c->lp, (uint64_t)nchunks * ncell * 4));
        HIP_TRY(launch_expand_hist(c->W, c->rsrc, c->chunks.as<Chunk>(), nchunks, k, F,
                                   c->lp.as<uint32_t>(), s));
        HIP_TRY(launch_cell_prefix(c->bin_chunk_begin.as<uint32_t>(), c->nlb, F, c->lp.as<uint32_t>(),
                                   c->cell_total.as<uint64_t>(), s));
    }
    HIP_TRY(scan_excl_sum_u64(c->cell_total.as<uint64_t>(), cell_base, ncell_all, cell_base + ncell_all, *on.ws, s));
    if (cut) HIP_TRY(hipEventRecord(c->side_ev[2], s));  // the cell totals and offsets are ready
    if (two_level) {
        FK_TRY(ensure(c->mid, total_kmers * 8 * c->KW));
        HIP_TRY(launch_expand_two_level(c->KW, c->rsrc, c->chunks.as<Chunk>(), nchunks, c->nlb, k, F,
                                        F2, c->lp.as<uint32_t>(), cell_base, c->mid.as<uint64_t>(),
                                        keys.as<uint64_t>(), s, c->x2_l1, total_kmers));
    } else {
        HIP_TRY(launch_expand_scatter(c->W, c->rsrc, c->chunks.as<Chunk>(), nchunks, k, F,
                                      c->lp.as<uint32_t>(), cell_base, keys.as<uint64_t>(), s));
    }
    return FK_OK;
}

// The buffers of one bucket cut and its counts.
struct CountBufs {
    DevBuf *flags, *flag_scan, *buckets, *bucket_unique, *tier_list, *piece_starts, *out_counts;
};
static CountBufs main_bufs(fk_ctx *c) {
    return CountBufs{&c->flags, &c->flag_scan, &c->buckets, &c->bucket_unique, &c->tier_list, &c->piece_starts,
                     &c->out_counts};
}

// 4c + 5: one count of a job's buckets -- the cut of the cells (ncell_all of them) into buckets, then
// every bucket's exact count from `src` (one key array, or the staged pieces') into okb / out_counts
// at the bucket's first slot, its distinct keys in bucket_unique.  What the steps below share:
struct BucketCount {
    fk_ctx *c;
    BucketSrc src;  // the cut sets F and the staged pieces' starts
    CountBufs B;
    DevBuf &okb;
    int k;
    uint32_t cap;  // keys of the largest bucket one workgroup's LDS holds
    // useHT=1 (extractKXmersHT, SBKC:664-739): the wave tiers' LDS hash tables emit their keys in
    // table order (the reference writes its hash map's iteration order, SBKC:723-734), no rank; the
    // heavier tiers' outputs stay ascending, which is one such order too
    bool ordered;
    // s: the wave tier, and the result after it.  cut: the bucket cut -- s, or the side stream beside
    // the last staged piece's expansion.  heavy: the tiers above the wave tier, on the side stream
    // (both with s's workspace: StreamWs)
    StreamWs s, cut, heavy;
    uint64_t nbuckets = 0;
    // the tiers above the wave tier, read back from pinned memory behind the tier kernel:
    // lists[0 .. ntier[0]) the block tier's buckets (up to mid_cap() keys), lists[nbuckets ..
    // nbuckets + ntier[1]) the big tier's; listed_keys = their keys
    uint32_t *lists = nullptr;
    uint32_t ntier[2] = {0, 0};
    uint64_t listed_keys = 0;
    // what the 64-bit mid tier's first kernel and the split leave: the buckets for the 1024-key kernel
    // (mid_fb), for the block path (fbB) and for the big-table / streaming path (fbG)
    bool mid_wave = false;
    int mid_mode = 0;  // the mid tier's first kernel: 0 none, 1 key ranges, 2 whole buckets (fk_debug_tier_stats)
    uint32_t *mid_fb = nullptr, *fbB = nullptr, *fbG = nullptr;
    uint32_t nmidfb = 0, nfbB = 0, nfbG = 0;

    const Bucket *buckets() const { return B.buckets->as<Bucket>(); }
    uint64_t *out_keys() const { return okb.as<uint64_t>(); }
    uint32_t *out_counts() const { return B.out_counts->as<uint32_t>(); }
    uint64_t *unique() const { return B.bucket_unique->as<uint64_t>(); }
    uint32_t mid_cap() const { return c->KW == 1 ? WAVE_MID_CAP : WAVE128_MID_CAP; }
    unsigned int *mid_fb_count() const { return c->misc.as<unsigned int>() + 11; }
};

// 64- / 128-bit keys: the same launch with the other kernel (and its sub-bucket type)
static hipError_t launch_wave_tier(const BucketCount &t, hipStream_t s) {
    if (t.c->KW == 1)
        return launch_bucket_count64_wave(t.src, t.buckets(), t.nbuckets, t.k, t.out_keys(), t.out_counts(), t.unique(),
                                          nullptr, s, t.ordered);
    return launch_bucket_count128_wave(t.src, t.buckets(), t.nbuckets, t.k, t.out_keys(), t.out_counts(), t.unique(), s,
                                       t.ordered);
}
static hipError_t launch_wave_mid(const BucketCount &t, const uint32_t *list, uint32_t n, hipStream_t s) {
    if (t.c->KW == 1)
        return launch_bucket_count64_wave_mid(t.src, t.buckets(), list, n, t.k, t.out_keys(), t.out_counts(), t.unique(),
                                              s, t.ordered);
    return launch_bucket_count128_wave_mid(t.src, t.buckets(), list, n, t.k, t.out_keys(), t.out_counts(), t.unique(), s,
                                           t.ordered);
}
static hipError_t launch_split(const BucketCount &t, const uint32_t *l1, uint32_t nl, SubBucket *subs,
                               unsigned int *counts, uint32_t *fb, hipStream_t s) {
    fk_ctx *c = t.c;
    return launch_bucket_split64(t.src, t.buckets(), t.lists, 0, l1, nl, c->sp_base.as<uint64_t>(),
                                 c->sp_keys.as<uint64_t>(), subs, c->sp_par.as<SplitParent>(), counts, fb, fb + nl,
                                 t.cap, t.k, t.src.F, s, c->split_retry);
}
static hipError_t launch_split(const BucketCount &t, const uint32_t *l1, uint32_t nl, SubBucket128 *subs,
                               unsigned int *counts, uint32_t *fb, hipStream_t s) {
    fk_ctx *c = t.c;
    return launch_bucket_split128(t.src, t.buckets(), l1, nl, c->sp_base.as<uint64_t>(), c->sp_keys.as<uint64_t>(), subs,
                                  c->sp_par.as<SplitParent>(), counts, fb, fb + nl, t.cap, t.k, t.src.F, s,
                                  c->split_retry);
}
static hipError_t launch_sub_count_seq(const BucketCount &t, const uint32_t *l1, uint32_t nl, const SubBucket *subs,
                                       hipStream_t s) {
    return launch_sub_count64_seq(t.buckets(), l1, nl, t.c->sp_par.as<SplitParent>(), subs, t.c->sp_keys.as<uint64_t>(),
                                  t.k, t.src.weighted, t.out_keys(), t.out_counts(), t.unique(), s, t.ordered);
}
static hipError_t launch_sub_count_seq(const BucketCount &t, const uint32_t *l1, uint32_t nl, const SubBucket128 *subs,
                                       hipStream_t s) {
    return launch_sub_count128_seq(t.buckets(), l1, nl, t.c->sp_par.as<SplitParent>(), subs, t.c->sp_keys.as<uint64_t>(),
                                   t.out_keys(), t.out_counts(), t.unique(), s, t.ordered);
}

// The listed buckets of at most cap keys in one workgroup's LDS: the block kernel (64-bit keys) or
// the LDS radix sort (128-bit keys).
static int block_tier(const BucketCount &t, const uint32_t *list, uint32_t n, hipStream_t s) {
    fk_ctx *c = t.c;
    if (c->KW == 1)
        HIP_TRY(launch_bucket_count64(t.src, t.buckets(), n, t.k, t.out_keys(), t.out_counts(), t.unique(),
                                      c->misc.as<unsigned long long>() + 1, t.cap, 99, list, s, 0));
    else
        HIP_TRY(launch_bucket_sort(2, t.src, t.buckets(), n, t.k, t.out_keys(), t.out_counts(), t.unique(),
                                   c->misc.as<unsigned long long>() + 1, t.cap, list, s, 0));
    return FK_OK;
}

// 4c: buckets.  Tiered (k <= 63): cells packed greedily into buckets of <= wave_cap keys for the wave
// kernel, larger cells to the tiers above it.  Otherwise buckets of <= cap keys.
static int bucket_cut(BucketCount &t, const SortedPlan &pl, uint64_t total_kmers, const uint64_t *cell_total,
                      const uint64_t *cell_base) {
    fk_ctx *c = t.c;
    const CountBufs &B = t.B;
    const hipStream_t cs = t.cut.s;
    const int F = pl.F;
    const uint32_t cap = pl.cap;
    const uint64_t ncell_all = (uint64_t)c->nlb << F;
    FK_TRY(ensure(*B.flags, ncell_all * 4));
    FK_TRY(ensure(*B.flag_scan, (ncell_all + 1) * 8));
    FK_TRY(ensure(c->misc, 64));
    if (pl.tiered)
        HIP_TRY(launch_bucket_flags_greedy(cell_total, c->nlb, F, pl.wave_cap, -1, B.flags->as<uint32_t>(), cs));
    else
        HIP_TRY(launch_bucket_flags(cell_base, cell_total, c->nlb, F, cap / 4, cap - cap / 4, B.flags->as<uint32_t>(), cs));
    HIP_TRY(scan_excl_sum_u32_to_u64(B.flags->as<uint32_t>(), B.flag_scan->as<uint64_t>(), ncell_all,
                                     B.flag_scan->as<uint64_t>() + ncell_all, *t.cut.ws, cs));
    uint64_t nbuckets = 0;
    HIP_TRY(hipMemcpyAsync(&nbuckets, B.flag_scan->as<uint64_t>() + ncell_all, 8, hipMemcpyDeviceToHost, cs));
    HIP_TRY(hipStreamSynchronize(cs));
    htrace("sorted: nbuckets read");
    t.nbuckets = nbuckets;
    FK_TRY(ensure(*B.buckets, nbuckets * sizeof(Bucket)));
    FK_TRY(ensure(t.okb, total_kmers * 8 * c->KW));
    FK_TRY(ensure(*B.out_counts, total_kmers * 4));
    FK_TRY(ensure(*B.bucket_unique, (nbuckets + 1) * 8));
    HIP_TRY(launch_bucket_write(cell_base, B.flags->as<uint32_t>(), B.flag_scan->as<uint64_t>(), c->nlb, F, nbuckets,
                                total_kmers, B.buckets->as<Bucket>(), cs));
    BucketSrc &src = t.src;
    src.F = F;
    if (src.np > 0) FK_TRY(ensure(*B.piece_starts, nbuckets * sizeof(PieceStarts)));
    // the buckets' sizes, and the staged pieces' starts per bucket (read by the wave tier)
    HIP_TRY(launch_bucket_finish(src, B.buckets->as<Bucket>(), nbuckets, c->nlb, cell_base + ncell_all,
                                 src.np > 0 ? B.piece_starts->as<PieceStarts>() : nullptr, cs));
    if (src.np > 0) src.starts = B.piece_starts->as<PieceStarts>();
    HIP_TRY(hipMemsetAsync(c->misc.p, 0, 64, cs));
    c->stats.buckets = nbuckets;
    c->stats.fine_bits = (uint64_t)F;
    c->stats.heavy_keys = 0;
    c->stats.split_buckets = c->stats.sub_buckets = 0;
    std::fill(c->tier_last, c->tier_last + 8, 0ull);
    return FK_OK;
}

// 5, tiered: the buckets above the wave tier listed by size, then every bucket of <= wave_cap keys on
// s.  The heavier tiers (split, in-order sub-buckets, mid wave tier, fallbacks) run on their own
// stream beside it: their buckets, outputs and counters are disjoint from its, and the host's waits
// for the split's counts do not wait for the wave tier.
static int wave_tier(BucketCount &t, uint32_t wave_cap) {
    fk_ctx *c = t.c;
    const hipStream_t s = t.s.s, cs = t.cut.s, hs = t.heavy.s;
    FK_TRY(ensure(*t.B.tier_list, t.nbuckets * 8));
    t.lists = t.B.tier_list->as<uint32_t>();
    // the block tier's top is the mid wave tier's cap; above it, the split (the 513..1024-key buckets
    // through the split as well, no mid wave tier: configs[2] load 1.1-1.4 ms slower, configs[1]
    // 0.3 ms, profiles/r05zg_mid_split_ab.txt)
    HIP_TRY(launch_bucket_tiers(t.buckets(), t.nbuckets, wave_cap, t.mid_cap(), t.unique(), t.lists,
                                c->misc.as<unsigned int>(), c->misc.as<unsigned long long>() + 3, cs));
    // the tier sizes (and the listed buckets' keys) go to pinned memory right behind the tier
    // kernel: the host waits for that copy, not for the wave tier queued after it, before it
    // queues the heavier tiers
    if (c->pin_tier.ensure(64)) return set_err(FK_E_NOMEM, "hipHostMalloc failed");
    HIP_TRY(hipMemcpyAsync(c->pin_tier.p, c->misc.p, 32, hipMemcpyDeviceToHost, cs));
    HIP_TRY(hipEventRecord(c->tier_ev, cs));
    if (cs != s) {  // the wave tier after the cut (and, in stream order, the last piece's expansion)
        HIP_TRY(hipEventRecord(c->side_ev[0], cs));
        HIP_TRY(hipStreamWaitEvent(s, c->side_ev[0], 0));
    }
    // the heavy tiers after both as well
    HIP_TRY(hipEventRecord(c->side_ev[3], s));
    HIP_TRY(hipStreamWaitEvent(hs, c->side_ev[3], 0));
    HIP_TRY(launch_wave_tier(t, s));
    HIP_TRY(hipEventSynchronize(c->tier_ev));
    t.ntier[0] = c->pin_tier.as<uint32_t>()[0], t.ntier[1] = c->pin_tier.as<uint32_t>()[1];
    t.listed_keys = c->pin_tier.as<uint64_t>()[3];
    htrace("sorted: tiers read");
    c->stats.heavy_keys = t.listed_keys;
    c->stats.block_buckets = t.ntier[0];
    c->stats.big_buckets = t.ntier[1];
    return FK_OK;
}

// The 64-bit mid tier (the block tier's buckets, 513 .. 1024 keys) on the wave tier's 512-key table,
// first on the side stream, ahead of the split: as 2 or 3 key ranges per bucket
// (k_bucket_count64_parts; the buckets it leaves, a range above 512 keys, are listed in mid_fb), only
// for a large mid tier: the configs[2] load's 278 K mid buckets 146.5 -> 146.2 ms, but configs[1]'s
// 59 K 21.8 -> 21.95 ms (profiles/r06v_mid_parts_ab.txt).  A smaller mid tier (a job whose k-mers
// repeat: configs[1]) goes on that table whole (k_bucket_count64_mid512), the buckets with more than
// 512 distinct keys listed in mid_fb.  FASTKMER_DEBUG_MID_PARTS = 0: neither (mid_tier_rest takes all).
static int mid_tier_first(BucketCount &t) {
    fk_ctx *c = t.c;
    constexpr uint32_t MID_PARTS_MIN = 1u << 17;  // mid-tier buckets from which the ranges kernel pays
    t.mid_wave = c->KW == 1 && t.ntier[0] && c->mid_parts != 0;
    if (!t.mid_wave) return FK_OK;
    const bool parts = c->mid_parts == 1 || (c->mid_parts != 2 && t.ntier[0] >= MID_PARTS_MIN);
    FK_TRY(ensure(c->mid_fb, (uint64_t)t.ntier[0] * 4));
    t.mid_fb = c->mid_fb.as<uint32_t>();
    t.mid_mode = parts ? 1 : 2;
    if (parts)
        HIP_TRY(launch_bucket_count64_parts(t.src, t.buckets(), t.lists, t.ntier[0], t.k, t.out_keys(), t.out_counts(),
                                            t.unique(), t.mid_fb, t.mid_fb_count(), t.heavy.s, t.ordered));
    else
        HIP_TRY(launch_bucket_count64_mid512(t.src, t.buckets(), t.lists, t.ntier[0], t.k, t.out_keys(),
                                             t.out_counts(), t.unique(), t.mid_fb, t.mid_fb_count(), t.heavy.s,
                                             t.ordered));
    return FK_OK;
}

#ifdef FK_PROBES
// FASTKMER_HOST_TRACE: the split buckets by size class (buckets, keys, fallbacks) and the wave
// tier's rank-loop counters before the split
static int split_probe_dump(const BucketCount &t, const uint32_t *l1, uint32_t nl, const uint32_t *fb,
                            const uint32_t *sc) {
    fk_ctx *c = t.c;
    std::vector<uint64_t> base((size_t)nl + 1);
    std::vector<uint32_t> f(2 * (size_t)nl), h_l((size_t)nl);
    HIP_TRY(hipMemcpy(base.data(), c->sp_base.p, base.size() * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(f.data(), fb, f.size() * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(h_l.data(), l1, (size_t)nl * 4, hipMemcpyDeviceToHost));
    std::unordered_map<uint32_t, uint32_t> pos;
    for (uint32_t j = 0; j < nl; ++j) pos[h_l[j]] = j;
    uint64_t hb[40] = {}, hk[40] = {}, hf[40] = {}, hfk[40] = {};
    std::vector<char> isfb(nl, 0);
    for (uint32_t j = 0; j < sc[1]; ++j) isfb[pos[f[j]]] = 1;
    for (uint32_t j = 0; j < sc[2]; ++j) isfb[pos[f[nl + j]]] = 1;
    for (uint32_t j = 0; j < nl; ++j) {
        const uint64_t n = base[j + 1] - base[j];
        const int cl = 63 - __builtin_clzll(n | 1);
        hb[cl] += 1, hk[cl] += n;
        if (isfb[j]) hf[cl] += 1, hfk[cl] += n;
    }
    unsigned long long rk[4];
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(rank_probe_read(rk, true));
    fprintf(stderr, "probe_rank (wave tier, before the split): iterations %llu keys %llu buckets %llu "
            "wall (small groups) %llu\n", rk[0], rk[1], rk[2], rk[3]);
    fprintf(stderr, "probe_split: split %u keys %llu subs %u fallbacks %u + %u\n", nl,
            (unsigned long long)base[nl], sc[0], sc[1], sc[2]);
    for (int cl = 0; cl < 40; ++cl)
        if (hb[cl])
            fprintf(stderr, "probe_split: n in [2^%d, 2^%d): buckets %llu keys %llu fallback buckets %llu keys %llu\n",
                    cl, cl + 1, (unsigned long long)hb[cl], (unsigned long long)hk[cl],
                    (unsigned long long)hf[cl], (unsigned long long)hfk[cl]);
    return FK_OK;
}
#endif

// The big tier (above the mid wave tier's cap) split into wave-sized sub-buckets by sampled splitters
// and counted in order by one wave per bucket; a bucket with a sub-bucket too large for a wave (a
// k-mer repeated that often) is left to the block kernel / LDS sort (fbB: <= cap keys) or to the
// big-table kernel (64-bit) and the streaming path (fbG).  Sub: SubBucket / SubBucket128.
template <typename Sub>
static int split_tier(BucketCount &t) {
    fk_ctx *c = t.c;
    const hipStream_t hs = t.heavy.s;
    const bool w1 = c->KW == 1;
    const uint32_t *l1 = t.lists + t.nbuckets;
    const uint32_t nl = t.ntier[1];
    const uint64_t maxsub = t.listed_keys / 64 + nl + 64;  // >= ceil(n / SPL_TGT) sub-buckets per bucket
    FK_TRY(ensure(c->sp_base, ((uint64_t)nl + 1) * 8));
    // 64-bit keys: a 512-key region per first-cut sub-bucket (split_room: <= 2 n + 512 per bucket)
    FK_TRY(ensure(c->sp_keys, (w1 ? 2 * t.listed_keys + 512ull * nl : t.listed_keys) * 8 * c->KW));
    FK_TRY(ensure(c->sp_subs, maxsub * sizeof(Sub)));
    FK_TRY(ensure(c->sp_par, (uint64_t)nl * sizeof(SplitParent)));
    FK_TRY(ensure(c->sp_fb, (uint64_t)nl * 8));
    uint32_t *fb = c->sp_fb.as<uint32_t>();
    unsigned int *spc = c->misc.as<unsigned int>() + 8;  // [0] sub-buckets, [1] / [2] fallbacks
    HIP_TRY(launch_listed_sizes(t.buckets(), t.lists, 0, l1, nl, c->sp_base.as<uint64_t>(), hs, w1));
    HIP_TRY(scan_excl_sum_u64(c->sp_base.as<uint64_t>(), c->sp_base.as<uint64_t>(), nl, c->sp_base.as<uint64_t>() + nl,
                              *t.heavy.ws, hs));
    HIP_TRY(launch_split(t, l1, nl, c->sp_subs.as<Sub>(), spc, fb, hs));
    HIP_TRY(hipMemcpyAsync(c->pin_tier.as<uint8_t>() + 32, spc, 16, hipMemcpyDeviceToHost, hs));
    HIP_TRY(hipEventRecord(c->tier_ev, hs));
    HIP_TRY(hipEventSynchronize(c->tier_ev));
    const uint32_t *sc = c->pin_tier.as<uint32_t>() + 8;
    const uint32_t nsub = sc[0];
    t.nmidfb = sc[3];  // misc word 11: the mid tier's leftovers (its kernel was queued before the copy)
    t.fbB = fb, t.nfbB = sc[1], t.fbG = fb + nl, t.nfbG = sc[2];
    htrace("sorted: split counts read");
#ifdef FK_PROBES
    if (w1 && getenv("FASTKMER_HOST_TRACE")) FK_TRY(split_probe_dump(t, l1, nl, fb, sc));
#endif
    if (nsub > maxsub)
        return set_err(FK_E_DEVICE, "bucket split: %u sub-buckets of at most %llu", nsub, (unsigned long long)maxsub);
    HIP_TRY(launch_sub_count_seq(t, l1, nl, c->sp_subs.as<Sub>(), hs));
    c->stats.split_buckets = nl - sc[1] - sc[2];
    c->stats.sub_buckets = nsub;
    return FK_OK;
}

// The block tier's buckets not yet counted, one wave each on the mid wave tier's table (64-bit keys:
// 1024 keys; 128-bit: 512): what mid_tier_first left, or all of them
static int mid_tier_rest(BucketCount &t) {
    fk_ctx *c = t.c;
    const hipStream_t hs = t.heavy.s;
    if (t.mid_wave && !t.ntier[1]) {  // no split read-back: the leftovers' count alone
        HIP_TRY(hipMemcpyAsync(c->pin_tier.as<uint8_t>() + 44, t.mid_fb_count(), 4, hipMemcpyDeviceToHost, hs));
        HIP_TRY(hipEventRecord(c->tier_ev, hs));
        HIP_TRY(hipEventSynchronize(c->tier_ev));
        t.nmidfb = c->pin_tier.as<uint32_t>()[11];
    }
    if (t.mid_wave) {
        if (t.nmidfb) HIP_TRY(launch_wave_mid(t, t.mid_fb, t.nmidfb, hs));
    } else if (t.ntier[0]) {
        HIP_TRY(launch_wave_mid(t, t.lists, t.ntier[0], hs));
    }
    return FK_OK;
}

// What the split left: the block kernel / LDS sort (<= cap keys), the big-table kernel (64-bit keys:
// above 2048 keys with at most 4096 distinct in one workgroup's LDS; the others stay REDO) and the
// streaming path.  *nlarge = buckets on the streaming path.
static int fallback_tiers(BucketCount &t, uint64_t *nlarge) {
    fk_ctx *c = t.c;
    const hipStream_t hs = t.heavy.s;
    if (t.nfbB) FK_TRY(block_tier(t, t.fbB, t.nfbB, hs));
    if (t.nfbG && c->KW == 1) {
        HIP_TRY(launch_bucket_count64_big(t.src, t.buckets(), t.nfbG, t.k, t.out_keys(), t.out_counts(), t.unique(),
                                          c->misc.as<unsigned long long>() + 2, t.fbG, hs));
        HIP_TRY(hipMemcpyAsync(nlarge, c->misc.as<unsigned long long>() + 2, 8, hipMemcpyDeviceToHost, hs));
        HIP_TRY(hipStreamSynchronize(hs));
    } else if (t.nfbG) {
        *nlarge = t.nfbG;  // 128-bit keys: no big-table kernel
    }
    if (*nlarge) {  // scratch for the listed buckets' keys only, taken by a cursor
        FK_TRY(ensure(c->scratch, t.listed_keys * 8 * c->KW));
        HIP_TRY(hipMemsetAsync(c->misc.as<unsigned long long>() + 6, 0, 8, hs));
        HIP_TRY(launch_bucket_sort_large(c->KW, t.src, t.buckets(), t.nfbG, t.k, c->scratch.as<uint64_t>(), t.out_keys(),
                                         t.out_counts(), t.unique(), t.fbG, hs,
                                         c->misc.as<unsigned long long>() + 6));
    }
    return FK_OK;
}

// 5, k = 64 and the streaming-path test hook: every bucket by one workgroup (<= small_limit keys in
// its LDS), the others on the streaming path
static int whole_bucket_tier(BucketCount &t, uint64_t total_kmers) {
    fk_ctx *c = t.c;
    const hipStream_t s = t.s.s;
    const uint32_t small_limit = c->force_large ? 0u : t.cap;
    if (t.src.np > 0) return set_err(FK_E_INVALID, "staged pieces need the tiered count");
    if (c->KW == 1)
        HIP_TRY(launch_bucket_count64(t.src, t.buckets(), t.nbuckets, t.k, t.out_keys(), t.out_counts(), t.unique(),
                                      c->misc.as<unsigned long long>(), small_limit, bucket_probe_phase(c), nullptr, s));
    else
        HIP_TRY(launch_bucket_sort(c->KW, t.src, t.buckets(), t.nbuckets, t.k, t.out_keys(), t.out_counts(), t.unique(),
                                   c->misc.as<unsigned long long>(), small_limit, nullptr, s));
    uint64_t oversize = 0;
    HIP_TRY(hipMemcpyAsync(&oversize, c->misc.p, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    c->stats.oversize_buckets = oversize;
    c->tier_last[3] = oversize;
    if (oversize) {
        FK_TRY(ensure(c->scratch, total_kmers * 8 * c->KW));
        HIP_TRY(launch_bucket_sort_large(c->KW, t.src, t.buckets(), t.nbuckets, t.k, c->scratch.as<uint64_t>(),
                                         t.out_keys(), t.out_counts(), t.unique(), nullptr, s));
    }
    return FK_OK;
}

// The steps in order.  `cut` (or null): the side stream for the bucket cut, beside the last staged
// piece's expansion on `on`.
static int sorted_count_buckets(fk_ctx *c, StreamWs on, hipStream_t cut, const SortedPlan &pl, const BucketSrc &src,
                                uint64_t total_kmers, const uint64_t *cell_total, const uint64_t *cell_base,
                                CountBufs B, DevBuf &okb, uint64_t *nb_out) {
    BucketCount t{c, src, B, okb, c->cfg.k, pl.cap, !c->cfg.use_ht,
                  on, StreamWs{cut ? cut : on.s, on.ws}, StreamWs{c->tier_side, on.ws}};
    FK_TRY(bucket_cut(t, pl, total_kmers, cell_total, cell_base));
    *nb_out = t.nbuckets;
    if (!pl.tiered) return whole_bucket_tier(t, total_kmers);
    FK_TRY(wave_tier(t, pl.wave_cap));
    uint64_t nlarge = 0;
    if (t.ntier[0] || t.ntier[1]) {  // above the wave tier
        FK_TRY(mid_tier_first(t));
        if (t.ntier[1])  // nothing to split: no split kernels, no read-back
            FK_TRY(c->KW == 1 ? split_tier<SubBucket>(t) : split_tier<SubBucket128>(t));
        FK_TRY(mid_tier_rest(t));
        FK_TRY(fallback_tiers(t, &nlarge));
    }
    // the result's scans follow both streams
    HIP_TRY(hipEventRecord(c->side_ev[1], t.heavy.s));
    HIP_TRY(hipStreamWaitEvent(t.s.s, c->side_ev[1], 0));
    c->stats.oversize_buckets = nlarge;
    // the census of this count (fk_debug_tier_stats): figures the steps above read to the host anyway
    c->tier_last[0] = t.nmidfb, c->tier_last[1] = t.nfbB, c->tier_last[2] = t.nfbG, c->tier_last[3] = nlarge;
    c->tier_last[4] = (uint64_t)t.mid_mode;
    return FK_OK;
}

// The count's result from its buckets: dense_off = the exclusive scan of the distinct keys per bucket,
// bin_off per local bin (`flag_scan` of the bucket cut: a bin's first cell starts a bucket).  The
// result stays bucket-major (no compaction pass): readers gather a bin's buckets (fk_get_bin) or the
// whole result (fk_write_bins, materialize_dense).
static int sorted_result(fk_ctx *c, StreamWs on, int F, uint64_t nbuckets, DevBuf &okb, CountBufs B) {
    hipStream_t s = on.s;
    FK_TRY(ensure(c->dense_off, (nbuckets + 1) * 8));
    HIP_TRY(scan_excl_sum_u64(B.bucket_unique->as<uint64_t>(), c->dense_off.as<uint64_t>(), nbuckets,
                              c->dense_off.as<uint64_t>() + nbuckets, *on.ws, s));
    FK_TRY(ensure(c->bin_off, ((uint64_t)c->nlb + 1) * 8));
    c->distinct_pending = true;
    HIP_TRY(launch_bin_offsets(B.flag_scan->as<uint64_t>(), c->dense_off.as<uint64_t>(), c->nlb, F, nbuckets,
                               c->bin_off.as<uint64_t>(), s));
    c->gapped = true;
    c->dense_ready = false;
    c->res_keys = okb.as<uint64_t>();
    c->res_nbuckets = nbuckets;
    c->res_F = F;
    c->res_fs = B.flag_scan->as<uint64_t>();
    return FK_OK;
}

static int sorted_count(fk_ctx *c, StreamWs on, hipStream_t cut, const SortedPlan &pl, const BucketSrc &src,
                        uint64_t total_kmers) {
    // the two-level count writes its buckets' results over the first expansion level (`mid` is dead
    // once level 2 has run, stream order; a staged job's `mid` held one piece and grows to the job
    // here, its contents dead): one k-mer array less on the device (57 GB at configs[3]'s per-GPU
    // load, 128-bit keys; 36 GB at configs[2]'s)
    DevBuf &okb = pl.two_level ? c->mid : c->out_keys;
    uint64_t nb = 0;
    int rc = sorted_count_buckets(c, on, cut, pl, src, total_kmers, c->cell_total.as<uint64_t>(),
                                  c->cell_base.as<uint64_t>(), main_bufs(c), okb, &nb);
    if (rc == FK_OK) rc = sorted_result(c, on, pl.F, nb, okb, main_bufs(c));
    // a failed count leaves nothing running on the side stream: its kernels read and write buffers
    // that the next job reuses (on success the main stream has waited for it, side_ev[1])
    if (rc != FK_OK) (void)hipStreamSynchronize(c->tier_side);
    return rc;
}


// After the bin offsets are on the host: the sorted count's distinct total is their last entry.
static void resolve_distinct(fk_ctx *c) {
    if (c->distinct_pending && !c->h_bin_off.empty()) c->distinct = c->h_bin_off.back();
    c->distinct_pending = false;
}

static int reduce_sorted(fk_ctx *c, StreamWs on, uint32_t nchunks, uint64_t total_kmers, uint64_t max_bin_kmers) {
    const SortedPlan pl = sorted_plan(c, max_bin_kmers);
    FK_TRY(sorted_expand(c, on, nullptr, pl, nchunks, total_kmers, c->keys, c->cell_base));
    BucketSrc src{c->keys.as<uint64_t>(), pl.F};
    return sorted_count(c, on, nullptr, pl, src, total_kmers);
}

// The end of a count queued on s: its bin offsets read back (the distinct total with them).
static int read_bin_offsets(fk_ctx *c, hipStream_t s) {
    const uint32_t nlb = c->nlb;
    c->h_bin_off.assign((size_t)nlb + 1, 0);
    if (c->pin_down.ensure(((size_t)nlb + 1) * 8)) return set_err(FK_E_NOMEM, "hipHostMalloc failed");
    HIP_TRY(hipMemcpyAsync(c->pin_down.p, c->bin_off.p, ((uint64_t)nlb + 1) * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    memcpy(c->h_bin_off.data(), c->pin_down.p, ((size_t)nlb + 1) * 8);
    resolve_distinct(c);
    return FK_OK;
}
// ... and the stats every count ends with (ms_partition, ms_count: the caller's)
static void count_done(fk_ctx *c, uint64_t nrecv, double t0) {
    c->stats.records_received = nrecv;
    c->stats.distinct = c->distinct;
    c->stats.ms_total += now_ms() - t0;
    c->have_result = true;
}

// Chunks of <= CHUNK_RECORDS records per local bin (chunks never span bins;
// a bin's chunks are consecutive).  ranges[lb] = the bin's record ranges.
static void build_chunks(uint32_t nlb, const std::vector<std::vector<std::pair<uint64_t, uint64_t>>> &ranges,
                         std::vector<Chunk> &chunks, std::vector<uint32_t> &bcb) {
    chunks.clear();
    bcb.assign((size_t)nlb + 1, 0);
    for (uint32_t lb = 0; lb < nlb; ++lb) {
        bcb[lb] = (uint32_t)chunks.size();
        for (const auto &rg : ranges[lb]) {
            for (uint64_t r = rg.first; r < rg.second; r += CHUNK_RECORDS) {
                Chunk ch;
                ch.rec_begin = r;
                ch.rec_end = std::min<uint64_t>(r + CHUNK_RECORDS, rg.second);
                ch.lbin = lb;
                ch.pad = 0;
                chunks.push_back(ch);
            }
        }
    }
    bcb[nlb] = (uint32_t)chunks.size();
}

// The count over the chunk table (records at c->rsrc), bin offsets, stats.
static int reduce_tail(fk_ctx *c, uint64_t nrecv, const std::vector<Chunk> &chunks, const std::vector<uint32_t> &bcb,
                       const std::vector<uint64_t> &bkm, double t0) {
    const StreamWs on = c->main_on();
    hipStream_t s = on.s;
    const uint32_t nlb = c->nlb;
    const uint32_t nchunks = (uint32_t)chunks.size();
    uint64_t total_kmers = 0, max_bin = 0;
    for (uint32_t lb = 0; lb < nlb; ++lb) {
        total_kmers += bkm[lb];
        max_bin = std::max(max_bin, bkm[lb]);
    }
    HIP_TRY(hipEventRecord(c->ev[6], s));
    // the sorted count; useHT=1 (extractKXmersHT) the same with the wave tiers in table order
    FK_TRY(reduce_sorted(c, on, nchunks, total_kmers, max_bin));
    HIP_TRY(hipEventRecord(c->ev[7], s));
    FK_TRY(read_bin_offsets(c, s));
    htrace("tail: bin offsets read");
    c->stats.ms_partition = ev_ms(c->ev[4], c->ev[5]);
    c->stats.ms_count = ev_ms(c->ev[6], c->ev[7]);
    count_done(c, nrecv, t0);
    return FK_OK;
}

// the chunk table to the device, queued on s
static int upload_chunks(fk_ctx *c, hipStream_t s, const std::vector<Chunk> &chunks, const std::vector<uint32_t> &bcb) {
    const uint32_t nchunks = (uint32_t)chunks.size();
    FK_TRY(ensure(c->chunks, nchunks * sizeof(Chunk)));
    FK_TRY(ensure(c->bin_chunk_begin, ((uint64_t)c->nlb + 1) * 4));
    // the previous upload out of the staging buffer may still be queued (on the map stream, or on the
    // staging stream behind a step's transfer): wait for it before the host overwrites the buffer
    if (c->pin_up_busy) FK_TRY(comm_event_sync(c, c->pin_up_ev));
    c->pin_up_busy = false;
    const size_t cb = (size_t)nchunks * sizeof(Chunk), bb = ((size_t)c->nlb + 1) * 4;
    if (c->pin_up.ensure(cb + bb)) return set_err(FK_E_NOMEM, "hipHostMalloc(%zu) failed", cb + bb);
    memcpy(c->pin_up.p, chunks.data(), cb);
    memcpy(c->pin_up.as<uint8_t>() + cb, bcb.data(), bb);
    if (nchunks) HIP_TRY(hipMemcpyAsync(c->chunks.p, c->pin_up.p, cb, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(c->bin_chunk_begin.p, c->pin_up.as<uint8_t>() + cb, bb, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(c->pin_up_ev, s));
    c->pin_up_busy = true;
    c->h_bcb = bcb;
    return FK_OK;
}

// partition of the records of `src` (all owned by this rank) by local bin into c->precs (the
// count stage reads them at c->rsrc), the chunk table uploaded; bkm = k-mers per local bin.  Queued on `on`.
static int partition_src(fk_ctx *c, StreamWs on, const RecSrc &src, uint64_t &nrecv, std::vector<Chunk> &chunks,
                         std::vector<uint32_t> &bcb, std::vector<uint64_t> &bkm, hipEvent_t e0, hipEvent_t e1) {
    nrecv = src.nrec;  // tiled sources: an upper bound, the partition counts them
    hipStream_t s = on.s;
    const uint32_t nlb = c->nlb;
    HIP_TRY(hipEventRecord(e0, s));
    FK_TRY(part_count(c->part, src, 1, c->G, local_table(c), nlb, *on.ws, s));
    htrace("reduce_src: part_count queued");
    // the scatter needs only the device-side offsets: it is queued before the host reads the part
    // totals (the output sized for src.nrec, for tiled sources the slot count: an upper bound), so
    // the GPU scatters while the host builds and uploads the chunk table
    FK_TRY(ensure(c->precs, src.nrec * c->W * 8));
    FK_TRY(part_scatter(c->part, 1, c->G, local_table(c), c->precs.as<uint64_t>(), s));
    htrace("reduce_src: scatter queued");
    std::vector<uint64_t> brec(nlb);
    bkm.assign(nlb, 0);
    if (c->pin_down.ensure((size_t)nlb * 16 + 16)) return set_err(FK_E_NOMEM, "hipHostMalloc failed");
    if (nlb) {
        HIP_TRY(hipMemcpyAsync(c->pin_down.p, c->part.rec.p, nlb * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(c->pin_down.as<uint64_t>() + nlb, c->part.kmer.p, nlb * 8, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    if (nlb) {
        memcpy(brec.data(), c->pin_down.p, nlb * 8);
        memcpy(bkm.data(), c->pin_down.as<uint64_t>() + nlb, nlb * 8);
    }
    htrace("reduce_src: part counts read");
    // the bins' records are consecutive after the partition: chunks straight from the bin totals (no
    // per-bin range lists: the host is on the critical path between the read-back and the upload)
    uint64_t off = 0, nch = 0;
    for (uint32_t lb = 0; lb < nlb; ++lb) {
        off += brec[lb];
        nch += (brec[lb] + CHUNK_RECORDS - 1) / CHUNK_RECORDS;
    }
    if (src.tcnt) {
        // a tiled source (the fused map's slots) holds this rank's own input, all of it owned only
        // with one rank; its record total is the partition's
        if (c->G != 1) return set_err(FK_E_STATE, "tiled records partitioned on a context of %u ranks", c->G);
        nrecv = off;
    }
    if (off != nrecv)
        return set_err(FK_E_INVALID, "received records belong to bins of another rank (%llu of %llu owned)",
                       (unsigned long long)off, (unsigned long long)nrecv);
    chunks.resize(nch);
    bcb.assign((size_t)nlb + 1, 0);
    off = 0;
    uint32_t ci = 0;
    for (uint32_t lb = 0; lb < nlb; ++lb) {
        bcb[lb] = ci;
        const uint64_t end = off + brec[lb];
        for (uint64_t r = off; r < end; r += CHUNK_RECORDS)
            chunks[ci++] = Chunk{r, std::min<uint64_t>(r + CHUNK_RECORDS, end), lb, 0u};
        off = end;
    }
    bcb[nlb] = ci;
    FK_TRY(upload_chunks(c, s, chunks, bcb));
    htrace("reduce_src: chunks uploaded");
    HIP_TRY(hipEventRecord(e1, s));
    c->rsrc = c->precs.as<uint64_t>();
    return FK_OK;
}

// reduce of the records of `src` (all owned by this rank): partition by local bin, then count
static int reduce_src(fk_ctx *c, const RecSrc &src) {
    const double t0 = now_ms();
    c->have_result = false;
    uint64_t nrecv = 0;
    std::vector<Chunk> chunks;
    std::vector<uint32_t> bcb;
    std::vector<uint64_t> bkm;
    FK_TRY(partition_src(c, c->main_on(), src, nrecv, chunks, bcb, bkm, c->ev[4], c->ev[5]));
    return reduce_tail(c, nrecv, chunks, bcb, bkm, t0);
}

FK_EXPORT int fk_reduce(fk_ctx *c, const void *d_recv, uint64_t nrecv) {
    if (!c) return set_err(FK_E_INVALID, "null ctx");
    DeviceGuard dg_(c->device);
    if (nrecv && !d_recv) return set_err(FK_E_INVALID, "null receive buffer");
    return reduce_src(c, dense_src((const uint64_t *)d_recv, nrecv, c->W));
}

FK_EXPORT int fk_set_grouped_emit(fk_ctx *c, int32_t enable) {
    if (!c) return set_err(FK_E_INVALID, "null ctx");
    DeviceGuard dg_(c->device);
    c->grouped = enable != 0;
    c->mapped = false;
    if (!c->grouped) return FK_OK;
    return build_group_table(c);
}

// The grouped emit's bin -> part table (part = destination * grp_nlb + the bin's local index there).
static int build_group_table(fk_ctx *c) {
    std::vector<uint32_t> table((size_t)c->Bc);
    if (c->custom_owners) {
        // size-aware placement (fk_set_bin_owners, the same table on every rank): part = owner *
        // L + the bin's index among its owner's bins in ascending order (the receiver's local bin)
        std::vector<uint32_t> cnt(c->G, 0);
        for (int32_t b = 0; b < c->Bc; ++b) table[b] = cnt[c->h_owner[b]]++;
        c->grp_nlb = std::max(1u, *std::max_element(cnt.begin(), cnt.end()));
        for (int32_t b = 0; b < c->Bc; ++b) table[b] += (uint32_t)c->h_owner[b] * c->grp_nlb;
    } else {
        c->grp_nlb = (uint32_t)((c->Bc + (int)c->G - 1) / (int)c->G);
        for (int32_t b = 0; b < c->Bc; ++b) table[b] = ((uint32_t)b % c->G) * c->grp_nlb + (uint32_t)b / c->G;
    }
    FK_TRY(ensure(c->grp_table, (uint64_t)c->Bc * 4));
    HIP_TRY(hipMemcpy(c->grp_table.p, table.data(), (uint64_t)c->Bc * 4, hipMemcpyHostToDevice));
    return FK_OK;
}

FK_EXPORT int32_t fk_grouped_parts_per_rank(const fk_ctx *c) { return c && c->grouped ? (int32_t)c->grp_nlb : 0; }

FK_EXPORT int fk_map_part_counts(fk_ctx *c, uint64_t *records, uint64_t *kmers) {
    if (!c || !records || !kmers) return set_err(FK_E_INVALID, "null argument");
    if (!c->grouped || !c->mapped) return set_err(FK_E_STATE, "fk_map_part_counts needs fk_set_grouped_emit and fk_map");
    std::copy(c->grp_rec.begin(), c->grp_rec.end(), records);
    std::copy(c->grp_kmer.begin(), c->grp_kmer.end(), kmers);
    return FK_OK;
}

// Counts records that arrive grouped by local bin: ranges[lb] = the bin's record ranges in d_recv.
static int reduce_ranges(fk_ctx *c, const uint64_t *d_recv, uint64_t nrecv,
                         const std::vector<std::vector<std::pair<uint64_t, uint64_t>>> &ranges,
                         const std::vector<uint64_t> &bkm, double t0) {
    std::vector<Chunk> chunks;
    std::vector<uint32_t> bcb;
    build_chunks(c->nlb, ranges, chunks, bcb);
    FK_TRY(upload_chunks(c, c->stream, chunks, bcb));
    HIP_TRY(hipEventRecord(c->ev[5], c->stream));
    c->rsrc = d_recv;
    return reduce_tail(c, nrecv, chunks, bcb, bkm, t0);
}

FK_EXPORT int fk_reduce_grouped(fk_ctx *c, const void *d_recv, uint64_t nrecv, const uint64_t *seg_records,
                                const uint64_t *seg_kmers, int32_t nseg, int32_t parts_per_seg) {
    if (!c) return set_err(FK_E_INVALID, "null ctx");
    DeviceGuard dg_(c->device);
    if (nrecv && !d_recv) return set_err(FK_E_INVALID, "null receive buffer");
    if (nseg < 0 || parts_per_seg < 0 || (nseg && (!seg_records || !seg_kmers)))
        return set_err(FK_E_INVALID, "bad segment table");
    const double t0 = now_ms();
    hipStream_t s = c->stream;
    c->have_result = false;
    const uint32_t nlb = c->nlb;
    if ((uint32_t)parts_per_seg < nlb) return set_err(FK_E_INVALID, "%d parts per segment < %u local bins",
                                                      parts_per_seg, nlb);
    HIP_TRY(hipEventRecord(c->ev[4], s));
    // segment s holds, bin after bin, seg_records[s * parts + lb] records of local bin lb
    std::vector<std::vector<std::pair<uint64_t, uint64_t>>> ranges(nlb);
    std::vector<uint64_t> bkm(nlb, 0);
    uint64_t off = 0;
    for (int32_t sg = 0; sg < nseg; ++sg) {
        for (int32_t lb = 0; lb < parts_per_seg; ++lb) {
            const uint64_t n = seg_records[(uint64_t)sg * parts_per_seg + lb];
            if (n && (uint32_t)lb >= nlb) return set_err(FK_E_INVALID, "records for local bin %d of %u", lb, nlb);
            if (n) {
                ranges[lb].push_back({off, off + n});
                bkm[lb] += seg_kmers[(uint64_t)sg * parts_per_seg + lb];
            }
            off += n;
        }
    }
    if (off != nrecv)
        return set_err(FK_E_INVALID, "segment table holds %llu records, buffer %llu", (unsigned long long)off,
                       (unsigned long long)nrecv);
    return reduce_ranges(c, (const uint64_t *)d_recv, nrecv, ranges, bkm, t0);
}

// ---------------------------------------------------------------------------
// staged pieces: a job's input partitioned and expanded piece by piece while later pieces land
// ---------------------------------------------------------------------------

// Staged pieces per job: 128-bit keys at most STAGE_MAXP128 (their kernels' piece loops stop there)
static uint32_t stage_maxp(const fk_ctx *c) { return c->KW == 2 ? (uint32_t)STAGE_MAXP128 : (uint32_t)STAGE_MAXP; }
// one rank's piece ends: FASTKMER_PIECE_CUTS, five pieces for a 64-bit job of >= 4 GB, else four
static const std::vector<double> &local_cuts(const fk_ctx *c) {
    if (!c->cuts_env && c->KW == 1 && c->job.job_bytes >= (4ull << 30) && STAGE_MAXP >= 5) return c->st_cuts5;
    return c->st_cuts;
}

static bool staged_eligible(const fk_ctx *c) { return staged_ok(c) && c->G == 1 && !c->comm; }

// Partitions one piece and expands it into its own key array (st_keys[p], its cells' exclusive
// scan in st_cb[p]); the job's cell totals accumulate in st_total.  The first piece fixes the
// job's cells: its largest bin scaled by the job's size over the bytes mapped so far.
// Expands one piece's records (the chunk table at c->chunks, records at c->rsrc; bkm = k-mers per
// local bin) into its own key array (st_keys[p], its cells' exclusive scan in st_cb[p]); the job's
// cell totals accumulate in st_total.  `frac` = the piece's estimated fraction of the job (0:
// unknown).  The first piece fixes the job's cells: its largest bin scaled to the job.  Queued on
// `on`; `cut` (or null, the last piece only): the side stream that sums the job's cell totals, and
// then cuts its buckets, while the piece's keys are expanded.
static int staged_expand_chunks(fk_ctx *c, StreamWs on, hipStream_t cut, uint32_t nchunks,
                                const std::vector<uint64_t> &bkm, double frac) {
    hipStream_t s = on.s;
    const uint32_t p = c->job.st_np;
    uint64_t pk = 0, maxb = 0;
    for (uint64_t v : bkm) pk += v, maxb = std::max(maxb, v);
    if (pk == 0) return FK_OK;  // nothing to expand (the piece's records hold no k-mers)
    if (p == 0) {
        const double scale = frac > 0.0 ? std::max(1.0, 1.0 / frac) : 2.0;
        c->job.st_plan = sorted_plan(c, (uint64_t)((double)maxb * scale));
        if (!c->job.st_plan.tiered || !c->job.st_plan.two_level)
            return set_err(FK_E_STATE, "staged pieces need the tiered two-level count");
    }
    // every piece takes both levels (level 2 sizes its workgroups to the keys per super-cell: a 15 %
    // piece 0.75 ms against 1.14 for a one-pass scatter)
    SortedPlan pl = c->job.st_plan;
    HIP_TRY(hipEventRecord(c->st_ev[4 * p + 2], s));
    FK_TRY(sorted_expand(c, on, cut, pl, nchunks, pk, c->st_keys[p], c->st_cb[p]));
    const uint64_t ncell_all = (uint64_t)c->nlb << c->job.st_plan.F;
    FK_TRY(ensure(c->st_total, ncell_all * 8));
    if (cut) {  // the job's cell totals on the cut's stream, while this piece is expanded
        HIP_TRY(hipStreamWaitEvent(cut, c->side_ev[2], 0));
        HIP_TRY(launch_add_u64(c->st_total.as<uint64_t>(), c->cell_total.as<uint64_t>(), ncell_all, p == 0, cut));
    } else {
        HIP_TRY(launch_add_u64(c->st_total.as<uint64_t>(), c->cell_total.as<uint64_t>(), ncell_all, p == 0, s));
    }
    HIP_TRY(hipEventRecord(c->st_ev[4 * p + 3], s));
    c->job.st_kmers += pk;
    c->job.st_np = p + 1;
    htrace("staged: piece expanded");
    return FK_OK;
}

// One rank: partitions a piece of the mapped tiles by local bin, then expands it.
static int staged_expand(fk_ctx *c, StreamWs on, hipStream_t cut, const RecSrc &src, double frac) {
    const uint32_t p = c->job.st_np;
    if (p >= stage_maxp(c)) return set_err(FK_E_STATE, "more than %u staged pieces", stage_maxp(c));
    uint64_t nrecv = 0;
    std::vector<Chunk> chunks;
    std::vector<uint32_t> bcb;
    std::vector<uint64_t> bkm;
    FK_TRY(partition_src(c, on, src, nrecv, chunks, bcb, bkm, c->st_ev[4 * p], c->st_ev[4 * p + 1]));
    return staged_expand_chunks(c, on, cut, (uint32_t)chunks.size(), bkm, frac);
}

// The job's count over the staged pieces: buckets over the summed cell totals, each bucket's keys
// read from every piece (BucketSrc pieces), the dense result and its bin offsets.  `cut` (or null):
// the side stream for the bucket cut, while the last piece is still being expanded on the main stream.
static int staged_count(fk_ctx *c, hipStream_t cut) {
    const double t0 = now_ms();
    const StreamWs on = c->main_on();
    hipStream_t s = on.s;
    const SortedPlan pl = c->job.st_plan;
    const uint32_t nlb = c->nlb;
    const uint64_t ncell_all = (uint64_t)nlb << pl.F;
    HIP_TRY(hipEventRecord(c->ev[6], s));
    std::swap(c->cell_total, c->st_total);  // the job's cell totals (st_total is rebuilt by the next job)
    FK_TRY(ensure(c->cell_base, (ncell_all + 1) * 8));
    // the bucket cut (this scan, then bucket_cut's flags, buckets and tiers) on the cut's stream
    const hipStream_t cs = cut ? cut : s;
    if (cut) HIP_TRY(hipStreamWaitEvent(cut, c->side_ev[2], 0));
    HIP_TRY(scan_excl_sum_u64(c->cell_total.as<uint64_t>(), c->cell_base.as<uint64_t>(), ncell_all,
                              c->cell_base.as<uint64_t>() + ncell_all, *on.ws, cs));
    BucketSrc src{nullptr, pl.F};
    src.np = (int)c->job.st_np;
    src.weighted = !c->job.fold_pieces.empty() || c->job.st_weighted;
    c->last_np = c->job.st_np, c->last_cells = ncell_all;
    for (uint32_t p = 0; p < c->job.st_np; ++p) {
        src.pk[p] = c->st_keys[p].as<uint64_t>();
        src.pcb[p] = c->st_cb[p].as<uint64_t>();
    }
    FK_TRY(sorted_count(c, on, cut, pl, src, c->job.st_kmers));
    HIP_TRY(hipEventRecord(c->ev[7], s));
    FK_TRY(read_bin_offsets(c, s));
    htrace("staged: bin offsets read");
    double mp = 0.0, mx = 0.0;
    for (uint32_t p = 0; p < c->job.st_np; ++p) {
        mp += ev_ms(c->st_ev[4 * p], c->st_ev[4 * p + 1]);
        mx += ev_ms(c->st_ev[4 * p + 2], c->st_ev[4 * p + 3]);
    }
    c->stats.ms_partition = mp;
    c->stats.ms_count = mx + ev_ms(c->ev[6], c->ev[7]);
    c->stats.pieces_counted = c->job.st_np;
    count_done(c, c->nrec, t0);
    return FK_OK;
}

// One rank: stages the tiles mapped since the last piece once they cover a piece (fk_ingest).
// The fused map's fallback flag is read first: a flagged input is counted whole by fk_finish.
// Piece ends: with the job's size known (one fk_ingest call, or fk_ingest_reserve) and no
// FASTKMER_PIECE_BYTES, at the fractions st_cuts of it (the last piece -- expanded after the last byte
// lands -- is the smallest); jobs under 2 * MIN_PIECE are counted whole.  A streamed job of unknown
// size: every piece_bytes, at most three pieces before fk_finish stages the last one (with cuts: at
// most stage_maxp - 1).
static bool local_piece_due(const fk_ctx *c, uint64_t tiles) {
    constexpr uint64_t MIN_PIECE = 256ull << 20;  // a piece holds >= half of it
    if (c->job.st_np >= stage_maxp(c) - 1) return false;
    const uint64_t tile = fm_tile_bytes(FUSED_NT);
    if (c->job.job_bytes && !c->piece_bytes_set) {
        const std::vector<double> &cuts = local_cuts(c);
        if (c->job.job_bytes < 2 * MIN_PIECE || c->job.st_cut >= cuts.size()) return false;
        const uint64_t end = (uint64_t)(cuts[c->job.st_cut] * (double)c->job.job_bytes);
        return tiles * tile >= end && (tiles - c->job.tiles_counted) * tile >= MIN_PIECE / 2;
    }
    // every piece_bytes: at most four pieces (three before fk_finish), as the exchange's
    return c->job.st_np < 3 && (tiles - c->job.tiles_counted) * tile >= c->piece_bytes;
}

// ---- the fold of a landed piece (fk_fold.inc)
// A job folds at all: one rank's staged pieces of 64-bit keys with a weight field (2k <= 60)
static bool fold_eligible(const fk_ctx *c) {
    return c->fold_mode != 0 && c->KW == 1 && 2 * c->cfg.k <= WKEY_MAX_BITS && staged_eligible(c);
}

// The gate of FASTKMER_FOLD=1, once per job behind its first piece's expansion: a count-only pass of
// the fold over one super-cell in FOLD_SAMPLE_STRIDE (an odd stride: a bin holds a power of two of
// them, and every 64th would be the same few of every bin; at most ~FOLD_SAMPLE_MAX super-cells, so
// that a large piece's sample stays a few tens of microseconds on a staging stream with no idle time:
// one in 61 of the configs[2] load's first piece took 0.25 ms) gives the entries per key the piece folds
// to; the job's pieces are folded when that ratio is at most FOLD_MAX_PPM.  The host waits for the
// figure (the piece's expansion): the copies and the maps of the whole call are queued already.
constexpr uint32_t FOLD_SAMPLE_STRIDE = 61;
constexpr uint64_t FOLD_SAMPLE_MAX = 4096;
constexpr uint64_t FOLD_MAX_PPM = 600000;
static int fold_decide(fk_ctx *c, StreamWs on, uint32_t p) {
    c->job.fold_decided = true;
    c->job.fold_on = c->fold_mode == 2;
    if (c->fold_mode != 1) return FK_OK;
    const SortedPlan &pl = c->job.st_plan;
    FK_TRY(ensure(c->fold_io, 16));
    const uint64_t nsc = (uint64_t)c->nlb << pl.F1;
    const uint32_t stride = (uint32_t)std::max<uint64_t>(FOLD_SAMPLE_STRIDE, (nsc / FOLD_SAMPLE_MAX) | 1ull);
    HIP_TRY(hipMemsetAsync(c->fold_io.p, 0, 16, on.s));
    HIP_TRY(launch_fold_sample(c->st_keys[p].as<uint64_t>(), c->st_cb[p].as<uint64_t>(), c->nlb, c->cfg.k, pl.F, pl.F2,
                               c->fold_wmax, stride, c->fold_io.as<unsigned long long>(), on.s));
    uint64_t io[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(io, c->fold_io.p, 16, hipMemcpyDeviceToHost, on.s));
    HIP_TRY(hipStreamSynchronize(on.s));
    c->job.fold_sample_ppm = io[0] ? io[1] * 1000000ull / io[0] : 1000000ull;
    c->job.fold_on = io[0] && c->job.fold_sample_ppm <= FOLD_MAX_PPM;
    htrace("staged: fold sampled");
    return FK_OK;
}

// The finished job's fold figures (fk_debug_fold_stats): pieces folded, their keys, their entries,
// the sample's entries per million keys.  counted = false: the pieces were dropped (counted whole).
static void fold_report(fk_ctx *c, bool counted) {
    uint64_t out = 0;
    for (uint32_t p : c->job.fold_pieces) out += c->fold_pin.as<uint64_t>()[p];
    c->fold_last[0] = counted ? c->job.fold_pieces.size() : 0;
    c->fold_last[1] = counted ? c->job.fold_in : 0;
    c->fold_last[2] = counted ? out : 0;
    c->fold_last[3] = c->job.fold_sample_ppm;
}

// Which pieces of a folding job (staged by local_maybe_piece, st_cut counting this one): with
// FASTKMER_FOLD=2 every one; else, of a job cut by its size, the first piece only.  A fold holds
// the staging stream, and only the first piece leaves it idle long enough (configs[1]: 3 ms between
// the end of its expansion and the next piece's last byte; the second piece's expansion ends 0.4 ms
// before the third lands): a later fold delays every piece behind it and, through them, the tail it
// was meant to shorten (profiles/r07_fold_c2_timeline_all_pieces.txt: the last piece 4.4 ms late).
static bool fold_piece_due(const fk_ctx *c) {
    if (c->fold_mode == 2) return true;
    if (c->job.job_bytes && !c->piece_bytes_set) return c->job.st_cut == 1;
    return true;
}

// Folds staged piece p (just expanded on `on`, pk keys): k_fold_sc into `mid` (dead since the piece's
// level 2), the scan of the entries per cell into the piece's new cell offsets, k_fold_compact back
// into st_keys[p]; st_total, which took the piece's raw cell totals, is corrected to the entries.
// The piece's raw k-mer count stays an upper bound of its entries wherever a size is needed.
static int fold_piece(fk_ctx *c, StreamWs on, uint32_t p, uint64_t pk) {
    if (pk == 0 || pk >= (1ull << 32)) return FK_OK;  // u32 entries per cell
    const SortedPlan &pl = c->job.st_plan;
    const uint64_t ncell_all = (uint64_t)c->nlb << pl.F;
    FK_TRY(ensure(c->fold_cnt, ncell_all * 4));
    FK_TRY(ensure(c->fold_cb, (ncell_all + 1) * 8));
    HIP_TRY(launch_fold_sc(c->st_keys[p].as<uint64_t>(), c->st_cb[p].as<uint64_t>(), c->nlb, c->cfg.k, pl.F, pl.F2,
                           c->fold_wmax, c->mid.as<uint64_t>(), c->fold_cnt.as<uint32_t>(), on.s));
    HIP_TRY(scan_excl_sum_u32_to_u64(c->fold_cnt.as<uint32_t>(), c->fold_cb.as<uint64_t>(), ncell_all,
                                     c->fold_cb.as<uint64_t>() + ncell_all, *on.ws, on.s));
    HIP_TRY(launch_fold_compact(c->mid.as<uint64_t>(), c->st_cb[p].as<uint64_t>(), c->fold_cb.as<uint64_t>(),
                                c->fold_cnt.as<uint32_t>(), c->nlb, pl.F, pl.F2, c->st_keys[p].as<uint64_t>(),
                                c->st_total.as<uint64_t>(), on.s));
    // the piece's entries, for fk_debug_fold_stats (read once the job is counted; nobody waits for it)
    if (c->fold_pin.ensure(8 * STAGE_MAXP)) return set_err(FK_E_NOMEM, "hipHostMalloc failed");
    HIP_TRY(hipMemcpyAsync(c->fold_pin.as<uint64_t>() + p, c->fold_cb.as<uint64_t>() + ncell_all, 8,
                           hipMemcpyDeviceToHost, on.s));
    std::swap(c->st_cb[p], c->fold_cb);  // stream order: the raw offsets are overwritten by the next fold's scan
    c->job.fold_in += pk;
    c->job.fold_pieces.push_back(p);
    htrace("staged: piece folded");
    return FK_OK;
}

// tiles: the tiles mapped once `mapped` (recorded on the map stream) has passed.  The piece is
// partitioned and expanded on the staging stream, which fk_finish joins (xstage_ev).
static int local_maybe_piece(fk_ctx *c, uint64_t tiles, hipEvent_t mapped) {
    if (!staged_eligible(c) || c->job.pieces_void || !local_piece_due(c, tiles)) return FK_OK;
    const StreamWs on = c->stage_on();
    hipStream_t s = on.s;
    HIP_TRY(hipStreamWaitEvent(s, mapped, 0));
    uint64_t h[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(h, c->counters.p, 32, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (h[2]) {
        c->job.pieces_void = true;
        return FK_OK;
    }
    const uint64_t t0 = c->job.tiles_counted, nt = tiles - t0;
    const RecSrc src = fused_src(c, t0, nt, nt * map_fused_tcap());
    c->job.tiles_counted = tiles;
    c->job.st_cut += 1;
    const uint32_t p = c->job.st_np;
    const uint64_t k0 = c->job.st_kmers;
    FK_TRY(staged_expand(c, on, nullptr, src,
                         c->job.job_bytes ? (double)(nt * fm_tile_bytes(FUSED_NT)) / (double)c->job.job_bytes : 0.0));
    // a piece staged here is never the job's last (fk_finish stages that one): fold it while the rest lands
    if (c->job.st_np > p && fold_eligible(c)) {
        if (!c->job.fold_decided) FK_TRY(fold_decide(c, on, p));
        if (c->job.fold_on && fold_piece_due(c)) FK_TRY(fold_piece(c, on, p, c->job.st_kmers - k0));
    }
    HIP_TRY(hipEventRecord(c->xstage_ev, s));
    return FK_OK;
}

// ---------------------------------------------------------------------------
// multi-rank exchange inside the context (fk_comm_init*)
// ---------------------------------------------------------------------------

enum : uint64_t { XF_FINAL = 1, XF_RETRACT = 2 };

// Host arithmetic of one exchange step (fk_exchange_plan): byte offsets and sizes of the send
// blocks (destination-major, as the grouped emit writes them) and of the receive blocks
// (sender-major), and whether every sender has sent its last piece.
static int plan_step(uint32_t G, uint32_t L, const uint64_t *sent, const uint64_t *got, uint64_t rb, uint64_t *soff,
                     uint64_t *sbytes, uint64_t *roff, uint64_t *rbytes, bool *all_final) {
    const size_t msg = 2 * (size_t)L + 1;
    uint64_t so = 0, ro = 0;
    bool fin = true;
    for (uint32_t d = 0; d < G; ++d) {
        uint64_t ns = 0, nr = 0;
        for (uint32_t lb = 0; lb < L; ++lb) {
            ns += sent[d * msg + lb];
            nr += got[d * msg + lb];
        }
        const uint64_t fs = sent[d * msg + 2 * L], fr = got[d * msg + 2 * L];
        if ((fs | fr) & ~(XF_FINAL | XF_RETRACT)) return set_err(FK_E_INVALID, "exchange step: unknown flag bits");
        if ((fr & XF_RETRACT) && !(fr & XF_FINAL))
            return set_err(FK_E_INVALID, "exchange step: rank %u retracts outside its last piece", d);
        fin = fin && (fr & XF_FINAL);
        soff[d] = so;
        sbytes[d] = ns * rb;
        roff[d] = ro;
        rbytes[d] = nr * rb;
        so += ns * rb;
        ro += nr * rb;
    }
    *all_final = fin;
    return FK_OK;
}

FK_EXPORT int fk_exchange_plan(int32_t n_ranks, int32_t parts, const uint64_t *sent, const uint64_t *received,
                               uint64_t record_bytes, uint64_t *send_off, uint64_t *send_bytes, uint64_t *recv_off,
                               uint64_t *recv_bytes, int32_t *all_final) {
    if (n_ranks < 1 || parts < 0 || !sent || !received || !send_off || !send_bytes || !recv_off || !recv_bytes ||
        !all_final)
        return set_err(FK_E_INVALID, "bad argument");
    bool fin = false;
    FK_TRY(plan_step((uint32_t)n_ranks, (uint32_t)parts, sent, received, record_bytes, send_off, send_bytes, recv_off,
                     recv_bytes, &fin));
    *all_final = fin ? 1 : 0;
    return FK_OK;
}

// FK_E_NOMEM from an exported call: the message names what the context holds on the device, largest
// first, so an oversized job shows which of its arrays to size (or free) without a re-run.
static int note_held(fk_ctx *c, int rc) {
    if (rc != FK_E_NOMEM || !c) return rc;
    std::vector<std::pair<size_t, std::string>> v;
    auto add = [&](const char *name, const DevBuf &b) {
        if (b.bytes >= (64u << 20)) v.emplace_back(b.bytes, name);
    };
#define FK_HELD(b) add(#b, c->b)
    FK_HELD(fasta_own); FK_HELD(rec_hdr); FK_HELD(rec_pos); FK_HELD(rec_code); FK_HELD(records);
    FK_HELD(codes); FK_HELD(valid); FK_HELD(precs); FK_HELD(chunks); FK_HELD(lp); FK_HELD(mid);
    FK_HELD(scratch); FK_HELD(keys); FK_HELD(out_keys); FK_HELD(out_counts); FK_HELD(buckets);
    FK_HELD(flags); FK_HELD(flag_scan); FK_HELD(cell_total); FK_HELD(cell_base); FK_HELD(dense_keys);
    FK_HELD(dense_counts); FK_HELD(bucket_unique);
    FK_HELD(sp_keys); FK_HELD(sp_subs); FK_HELD(xsend); FK_HELD(xrecv);
    add("gather_keys", c->vw.gather_keys); FK_HELD(part.K); FK_HELD(part.KT); FK_HELD(dest.K); FK_HELD(dest.KT);
#undef FK_HELD
    std::vector<std::string> piece_names(STAGE_MAXP);
    for (int p = 0; p < STAGE_MAXP; ++p) {
        piece_names[p] = "st_keys[" + std::to_string(p) + "]";
        add(piece_names[p].c_str(), c->st_keys[p]);
    }
    std::sort(v.rbegin(), v.rend());
    size_t total = 0;
    for (const auto &e : v) total += e.first;
    std::string msg = g_err + "; held on the device: " + std::to_string(total >> 20) + " MiB in";
    for (size_t i = 0; i < v.size() && i < 12; ++i)
        msg += (i ? ", " : " ") + v[i].second + " " + std::to_string(v[i].first >> 20) + " MiB";
    g_err = msg;
    return rc;
}

static int comm_fail(fk_ctx *c, int rc) {
    note_held(c, rc);
    if (c->comm) c->comm->abort();  // peers blocked in a step return instead of waiting
    return rc;
}

static hipEvent_t xch_event(fk_ctx *c, size_t i) {
    if (ensure_events(c->xev, i + 1) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return c->xev[i];
}

// One exchange step; collective (every rank runs its steps in the same sequence, whatever each
// step carries).  src = this rank's records of the step (null: none): grouped by (destination,
// local bin) into the send ring, their per-part counts and `flags` all-to-all'ed, then the
// records posted on the comm stream (they move while the map stream goes on); the received
// blocks become segments of the count.  `expect` = records expected in all (sizes xrecv).
static int xch_step(fk_ctx *c, const RecSrc *src, uint64_t flags) {
    hipStream_t s = c->stream, cs = c->comm_stream;
    const uint32_t G = c->G, L = c->grp_nlb, nparts = G * L;
    const uint64_t rb = (uint64_t)c->W * 8;
    const size_t msg = 2 * (size_t)L + 1;
    std::vector<uint64_t> pr(nparts, 0), pk(nparts, 0);
    uint64_t piece_rec = 0;
    if (src && src->nrec && src->ntiles) {
        FK_TRY(part_count(c->dest, *src, 0, G, c->grp_table.as<uint32_t>(), nparts, c->ws, s));
        HIP_TRY(hipMemcpyAsync(pr.data(), c->dest.rec.p, (uint64_t)nparts * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(pk.data(), c->dest.kmer.p, (uint64_t)nparts * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        for (uint64_t v : pr) piece_rec += v;
    }
    if (piece_rec) {
        // send ring: earlier pieces are read by the comm stream; wrap around once it has drained
        if ((c->job.xch.send_used + piece_rec) * rb > c->xsend.bytes) {
            FK_TRY(comm_sync(c, cs));
            c->job.xch.send_used = 0;
            FK_TRY(ensure(c->xsend, piece_rec * rb * 2));
        }
        FK_TRY(part_scatter(c->dest, 0, G, c->grp_table.as<uint32_t>(), c->xsend.as<uint64_t>() + c->job.xch.send_used * c->W,
                            s));
        HIP_TRY(hipEventRecord(c->emit_ev, s));
    }
    std::vector<uint64_t> out((size_t)G * msg), in((size_t)G * msg);
    for (uint32_t d = 0; d < G; ++d) {
        for (uint32_t lb = 0; lb < L; ++lb) {
            out[d * msg + lb] = pr[(size_t)d * L + lb];
            out[d * msg + L + lb] = pk[(size_t)d * L + lb];
        }
        out[d * msg + 2 * L] = flags;
    }
    std::string err;
    if (c->comm->alltoall_u64(out.data(), in.data(), msg, cs, err))
        return set_err(FK_E_COMM, "exchange step %llu, counts: %s", (unsigned long long)c->job.xch.pieces, err.c_str());
    std::vector<uint64_t> soff(G), sbytes(G), roff(G), rbytes(G);
    bool all_final = false;
    FK_TRY(plan_step(G, L, out.data(), in.data(), rb, soff.data(), sbytes.data(), roff.data(), rbytes.data(), &all_final));
    uint64_t recv_rec = 0;
    for (uint32_t r = 0; r < G; ++r) recv_rec += rbytes[r] / rb;
    if ((c->job.xch.recv_used + recv_rec) * rb > c->xrecv.bytes) {
        // the received records stay until the count: grow, keeping them (sized for the whole input
        // once the first pieces show the records per FASTA byte)
        uint64_t want = c->job.xch.recv_used + recv_rec;
        if (c->job.xch.expect_bytes && c->job.xch.tiles_sent) {
            const double covered = (double)c->job.xch.tiles_sent * (double)fm_tile_bytes(FUSED_NT);
            want = std::max<uint64_t>(want, (uint64_t)((double)want * (double)c->job.xch.expect_bytes / covered * 1.1));
        }
        FK_TRY(comm_sync(c, cs));
        FK_TRY(comm_sync(c, c->xstage));  // staged expansions may still read the old buffer
        FK_TRY(grow_keep(c->xrecv, want * rb, c->job.xch.recv_used * rb, s));
    }
    const size_t step = (size_t)c->job.xch.pieces;
    hipEvent_t e0 = xch_event(c, 2 * step), e1 = xch_event(c, 2 * step + 1);
    if (!e0 || !e1) return set_err(FK_E_DEVICE, "hipEventCreate failed");
    if (piece_rec) HIP_TRY(hipStreamWaitEvent(cs, c->emit_ev, 0));
    HIP_TRY(hipEventRecord(e0, cs));
    if (c->comm->alltoallv(c->xsend.as<uint8_t>() + c->job.xch.send_used * rb, soff.data(), sbytes.data(),
                           c->xrecv.as<uint8_t>() + c->job.xch.recv_used * rb, roff.data(), rbytes.data(), cs, err))
        return set_err(FK_E_COMM, "exchange step %llu, records: %s", (unsigned long long)step, err.c_str());
    HIP_TRY(hipEventRecord(e1, cs));
    for (uint32_t r = 0; r < G; ++r) {
        const uint64_t *m = in.data() + (size_t)r * msg;
        if (m[2 * L] & XF_RETRACT) {  // the sender mapped again from scratch: its earlier pieces are void
            c->job.pieces_void = true;      // (and so are the piece counts that hold them)
            auto &v = c->job.xch.segs;
            v.erase(std::remove_if(v.begin(), v.end(), [&](const fk_ctx::XSeg &g) { return g.sender == (int32_t)r; }),
                    v.end());
        }
        if (!rbytes[r]) continue;
        fk_ctx::XSeg g;
        g.off = c->job.xch.recv_used + roff[r] / rb;
        g.sender = (int32_t)r;
        g.step = step;
        g.rec.assign(m, m + L);
        g.kmer.assign(m + L, m + 2 * L);
        c->job.xch.segs.push_back(std::move(g));
        if (r != (uint32_t)c->cfg.rank) c->job.xch.bytes_received += rbytes[r];
    }
    for (uint32_t d = 0; d < G; ++d)
        if (d != (uint32_t)c->cfg.rank) c->job.xch.bytes_sent += sbytes[d];
    c->job.xch.send_used += piece_rec;
    c->job.xch.recv_used += recv_rec;
    c->job.xch.pieces += 1;
    c->job.xch.open = true;
    c->job.xch.all_final = all_final;
    if (flags & XF_FINAL) c->job.xch.sent_final = true;
    return FK_OK;
}

// Ranges of every local bin over the received segments [s0, s1) (each segment holds its
// records bin after bin).
static int segment_ranges(fk_ctx *c, size_t s0, size_t s1, std::vector<std::vector<std::pair<uint64_t, uint64_t>>> &ranges,
                          std::vector<uint64_t> &bkm, uint64_t *nrecv) {
    const uint32_t nlb = c->nlb;
    ranges.assign(nlb, {});
    bkm.assign(nlb, 0);
    *nrecv = 0;
    for (size_t i = s0; i < s1; ++i) {
        const fk_ctx::XSeg &g = c->job.xch.segs[i];
        uint64_t off = g.off;
        for (uint32_t lb = 0; lb < c->grp_nlb; ++lb) {
            const uint64_t n = g.rec[lb];
            if (n && lb >= nlb) return set_err(FK_E_INVALID, "records for local bin %u of %u", lb, nlb);
            if (n) {
                ranges[lb].push_back({off, off + n});
                bkm[lb] += g.kmer[lb];
                *nrecv += n;
            }
            off += n;
        }
    }
    return FK_OK;
}

// With a communicator and staged pieces: expands the received segments [segs_counted, s1) as one
// staged piece (they arrive grouped by local bin: no partition), once the comm stream has
// delivered them.  `frac` = their estimated fraction of what this rank receives in the job.
static int xch_stage_segments(fk_ctx *c, size_t s1, double frac) {
    if (s1 <= c->job.segs_counted) return FK_OK;
    const uint32_t p = c->job.st_np;
    if (p >= stage_maxp(c)) return set_err(FK_E_STATE, "more than %u staged pieces", stage_maxp(c));
    const StreamWs on = c->stage_on();
    hipStream_t s = on.s;
    // its earlier work (behind earlier steps' transfers) is done: bounded with a communicator
    FK_TRY(comm_sync(c, s));
    const uint64_t step = c->job.xch.segs[s1 - 1].step;
    HIP_TRY(hipStreamWaitEvent(s, c->xev[2 * step + 1], 0));
    std::vector<std::vector<std::pair<uint64_t, uint64_t>>> ranges;
    std::vector<uint64_t> bkm;
    uint64_t nrecv = 0;
    FK_TRY(segment_ranges(c, c->job.segs_counted, s1, ranges, bkm, &nrecv));
    c->job.segs_counted = s1;
    std::vector<Chunk> chunks;
    std::vector<uint32_t> bcb;
    build_chunks(c->nlb, ranges, chunks, bcb);
    HIP_TRY(hipEventRecord(c->st_ev[4 * p], s));
    FK_TRY(upload_chunks(c, s, chunks, bcb));
    HIP_TRY(hipEventRecord(c->st_ev[4 * p + 1], s));
    c->rsrc = c->xrecv.as<uint64_t>();
    return staged_expand_chunks(c, on, nullptr, (uint32_t)chunks.size(), bkm, frac);
}

// Received records of this job so far / expected in all (estimated from the share of the input
// sent so far; 0 when the input's size is unknown).
static double xch_recv_frac(const fk_ctx *c, uint64_t recs) {
    if (!c->job.xch.expect_bytes || !c->job.xch.tiles_sent || !c->job.xch.recv_used) return 0.0;
    const double sent = (double)c->job.xch.tiles_sent * (double)fm_tile_bytes(FUSED_NT);
    const double est = (double)c->job.xch.recv_used * (double)c->job.xch.expect_bytes / sent;
    return est > 0.0 ? std::min(1.0, (double)recs / est) : 0.0;
}

// Staged: the segments received before this step are expanded once they hold about 1 / STAGE_MAXP
// of the job (every step when its size is unknown), at most STAGE_MAXP - 1 times before fk_finish.
static int xch_maybe_stage(fk_ctx *c, size_t s1) {
    // (at most four pieces: the exchange's cuts are xst_cuts)
    if (c->job.st_np >= std::min<uint32_t>(stage_maxp(c), 4) - 1 || s1 <= c->job.segs_counted) return FK_OK;
    uint64_t recs = 0, before = 0;
    for (size_t i = 0; i < s1; ++i)
        for (uint64_t n : c->job.xch.segs[i].rec) (i < c->job.segs_counted ? before : recs) += n;
    const double frac = xch_recv_frac(c, recs);
    // a piece ends once the received records reach the next cut of the job (st_cuts, as the local
    // path's pieces): the last piece -- expanded after the last byte -- is the smallest.  (Staging at
    // every quarter left ~30 % of a 6.25 GB rank for fk_finish: 61.7 ms after it against 47.7 for
    // the local path, profiles/r04c_xch_tail.txt.)
    if (frac > 0.0) {
        if (c->job.st_np >= (uint32_t)c->xst_cuts.size()) return FK_OK;
        if (xch_recv_frac(c, before + recs) < c->xst_cuts[c->job.st_np]) return FK_OK;
    }
    return xch_stage_segments(c, s1, frac);
}

// fk_ingest: sends the tiles mapped since the last piece once they cover a piece.  The fused
// map's fallback flag is read first: a flagged input is mapped again in fk_finish and sent
// whole, retracting the pieces sent so far.
static int xch_maybe_piece(fk_ctx *c) {
    if (c->job.xch.stop_pieces || c->job.xch.sent_final) return FK_OK;
    const uint64_t tile = fm_tile_bytes(FUSED_NT);
    if ((c->job.pm_tiles - c->job.xch.tiles_sent) * tile < c->piece_bytes) return FK_OK;
    uint64_t h[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(h, c->counters.p, 32, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (h[2]) {
        c->job.xch.stop_pieces = true;
        return FK_OK;
    }
    const uint64_t t0 = c->job.xch.tiles_sent, nt = c->job.pm_tiles - t0;
    const RecSrc src = fused_src(c, t0, nt, nt * map_fused_tcap());
    c->job.xch.tiles_sent = c->job.pm_tiles;
    const int rc = xch_step(c, &src, 0);
    if (rc) return comm_fail(c, rc);
    // the received segments are expanded (staged) on the staging stream as soon as their transfer
    // ends, this step's included, while the map stream goes on
    if (staged_ok(c) && !c->job.pieces_void) FK_TRY(xch_maybe_stage(c, c->job.xch.segs.size()));
    return FK_OK;
}

// fk_finish with a communicator: the last piece, the closing steps, then the count of every
// received segment.
static int finish_exchange(fk_ctx *c) {
    const double t0 = now_ms();
    hipStream_t s = c->stream, cs = c->comm_stream;
    const bool pieced = c->job.xch.tiles_sent > 0;
    const uint64_t tiles_sent = c->job.xch.tiles_sent;
    FK_TRY(map_records(c));
    RecSrc src;
    uint64_t flags = XF_FINAL;
    if (c->rec_tiled && pieced && !c->job.xch.stop_pieces && tiles_sent <= c->rec_tiles) {
        const uint64_t nt = c->rec_tiles - tiles_sent;
        src = fused_src(c, tiles_sent, nt, nt * map_fused_tcap());
    } else {
        src = map_src(c);
        if (pieced) flags |= XF_RETRACT;
    }
    c->mapped = true;
    int rc = xch_step(c, &src, flags);
    const size_t last_step = (size_t)c->job.xch.pieces - 1;
    while (!rc && !c->job.xch.all_final) rc = xch_step(c, nullptr, XF_FINAL);
    // every transfer of the job has been posted; the host waits for them here, bounded, so that none
    // of the count's host waits below can block on a peer that died (FK_E_COMM instead)
    if (!rc) rc = comm_sync(c, cs);
    if (rc) return comm_fail(c, rc);
    HIP_TRY(hipEventRecord(c->ev[4], cs));  // every rank's records have landed
    HIP_TRY(hipStreamWaitEvent(s, c->ev[4], 0));
    HIP_TRY(hipEventRecord(c->xstage_ev, c->xstage));  // and the staged expansions queued so far are done
    HIP_TRY(hipStreamWaitEvent(s, c->xstage_ev, 0));
    uint64_t nrecv = 0;
    for (const auto &g : c->job.xch.segs)
        for (uint64_t n : g.rec) nrecv += n;
    if (c->job.st_np && !c->job.pieces_void) {
        // staged: the segments not yet expanded, then one count over every piece
        if (c->job.segs_counted < c->job.xch.segs.size()) {
            uint64_t recs = 0;
            for (size_t i = c->job.segs_counted; i < c->job.xch.segs.size(); ++i)
                for (uint64_t n : c->job.xch.segs[i].rec) recs += n;
            FK_TRY(xch_stage_segments(c, c->job.xch.segs.size(), nrecv ? (double)recs / (double)nrecv : 0.0));
            HIP_TRY(hipEventRecord(c->xstage_ev, c->xstage));
            HIP_TRY(hipStreamWaitEvent(s, c->xstage_ev, 0));
        }
        FK_TRY(staged_count(c, nullptr));
    } else {
        std::vector<std::vector<std::pair<uint64_t, uint64_t>>> ranges;
        std::vector<uint64_t> bkm;
        FK_TRY(segment_ranges(c, 0, c->job.xch.segs.size(), ranges, bkm, &nrecv));
        FK_TRY(reduce_ranges(c, c->xrecv.as<uint64_t>(), nrecv, ranges, bkm, t0));
    }
    end_pieces(c);
    // exchange figures (every transfer has completed: the count waited for them)
    double ms = 0.0;
    for (size_t i = 0; i < (size_t)c->job.xch.pieces; ++i) ms += ev_ms(c->xev[2 * i], c->xev[2 * i + 1]);
    c->stats.xch_steps = c->job.xch.pieces;
    c->stats.xch_bytes_sent = c->job.xch.bytes_sent;
    c->stats.xch_bytes_received = c->job.xch.bytes_received;
    c->stats.ms_exchange = ms;
    c->stats.ms_exchange_tail = ev_ms(c->xev[2 * last_step], c->xev[2 * ((size_t)c->job.xch.pieces - 1) + 1]);
    c->stats.records_received = nrecv;
    c->job.xch = fk_ctx::Xch{};
    return FK_OK;
}

static int finish_local(fk_ctx *c);

FK_EXPORT int fk_finish(fk_ctx *c) {
    htrace("fk_finish: enter");
    if (!c) return set_err(FK_E_INVALID, "null ctx");
    if (c->comm) {
        DeviceGuard dg_(c->device);
        const int rc = finish_exchange(c);
        return rc ? comm_fail(c, rc) : rc;  // collective: a failed rank fails the group
    }
    return note_held(c, finish_local(c));
}

static int finish_local(fk_ctx *c) {
    if (c->G != 1)
        return set_err(FK_E_STATE, "fk_finish over %u ranks needs a communicator (fk_comm_init); or use "
                                   "fk_map/fk_map_emit/fk_reduce", c->G);
    FK_TRY(fk_map(c, nullptr));  // joins the staging stream first
    DeviceGuard dg_(c->device);
    if (c->job.st_np && c->rec_tiled && !c->job.pieces_void && c->job.tiles_counted <= c->rec_tiles) {
        // staged pieces were expanded while the input landed: the last piece, then one count
        // the job's bucket cut needs the last piece's cell totals, not its keys: it runs on the side
        // stream while the piece's two expansion levels run on `stream`
        int rc = FK_OK;
        const hipStream_t cut = c->rec_tiles > c->job.tiles_counted ? c->tier_side : nullptr;
        // the cut's stream starts after everything queued so far (re-recorded once the last piece's cell
        // offsets are scanned; a piece without k-mers records nothing more)
        if (cut) HIP_TRY(hipEventRecord(c->side_ev[2], c->stream));
        if (c->rec_tiles > c->job.tiles_counted) {
            const uint64_t t0 = c->job.tiles_counted, nt = c->rec_tiles - t0;
            rc = staged_expand(c, c->main_on(), cut, fused_src(c, t0, nt, nt * map_fused_tcap()),
                               c->job.job_bytes ? (double)(nt * fm_tile_bytes(FUSED_NT)) / (double)c->job.job_bytes : 0.0);
        }
        if (rc == FK_OK) rc = staged_count(c, cut);
        if (cut) (void)hipStreamSynchronize(cut);
        FK_TRY(rc);
        fold_report(c, true);
        end_pieces(c);
        return FK_OK;
    }
    fold_report(c, false);
    end_pieces(c);
    return reduce_src(c, map_src(c));
}

static int attach_comm(fk_ctx *c, fk::Comm *comm) {
    DeviceGuard dg_(c->device);
    HIP_TRY(c->comm_stream.create());
    HIP_TRY(c->xstage.create());
    HIP_TRY(c->xstage_ev.create(hipEventDisableTiming));
    HIP_TRY(c->emit_ev.create(hipEventDisableTiming));
    c->comm = comm;
    if (!c->piece_bytes_set) c->piece_bytes = 1ull << 30;
    FK_TRY(fk_set_grouped_emit(c, 1));  // records leave grouped by (owner rank, local bin)
    c->job.xch = fk_ctx::Xch{};
    return FK_OK;
}

FK_EXPORT int fk_comm_unique_id(uint8_t *id) {
    if (!id) return set_err(FK_E_INVALID, "null argument");
    std::string err;
    if (fk::comm_unique_id(id, err)) return set_err(FK_E_DEVICE, "%s", err.c_str());
    return FK_OK;
}

FK_EXPORT int fk_comm_init(fk_ctx *c, const uint8_t *id) {
    if (!c || !id) return set_err(FK_E_INVALID, "null argument");
    if (c->comm) return set_err(FK_E_STATE, "the context already has a communicator");
    DeviceGuard dg_(c->device);
    std::string err;
    fk::Comm *comm = fk::comm_create_rccl(id, (int)c->G, c->cfg.rank, c->device, err);
    if (!comm) return set_err(FK_E_DEVICE, "%s", err.c_str());
    const int rc = attach_comm(c, comm);
    if (rc) {
        delete comm;
        c->comm = nullptr;
    }
    return rc;
}

FK_EXPORT int fk_comm_init_local(fk_ctx **ctxs, int32_t n) {
    if (!ctxs || n < 1) return set_err(FK_E_INVALID, "bad argument");
    std::vector<int> devs(n);
    for (int32_t r = 0; r < n; ++r) {
        fk_ctx *c = ctxs[r];
        if (!c) return set_err(FK_E_INVALID, "null context %d", r);
        if (c->G != (uint32_t)n || c->cfg.rank != r)
            return set_err(FK_E_INVALID, "context %d has rank %d of %u; expected rank %d of %d", r, c->cfg.rank, c->G,
                           r, n);
        if (c->comm) return set_err(FK_E_STATE, "context %d already has a communicator", r);
        devs[r] = c->device;
    }
    std::vector<fk::Comm *> comms(n, nullptr);
    std::string err;
    if (fk::comm_create_local(n, devs.data(), comms.data(), err)) return set_err(FK_E_DEVICE, "%s", err.c_str());
    for (int32_t r = 0; r < n; ++r) {
        const int rc = attach_comm(ctxs[r], comms[r]);
        if (rc) {
            for (int32_t q = 0; q < n; ++q) {
                if (ctxs[q]->comm == comms[q]) ctxs[q]->comm = nullptr;
                delete comms[q];
            }
            return rc;
        }
    }
    return FK_OK;
}

FK_EXPORT const char *fk_comm_transport(const fk_ctx *c) { return c && c->comm ? c->comm->kind() : ""; }

FK_EXPORT int fk_comm_allreduce_u64(fk_ctx *c, uint64_t *v, size_t n) {
    if (!c || (!v && n)) return set_err(FK_E_INVALID, "null argument");
    if (!c->comm) return set_err(FK_E_STATE, "fk_comm_allreduce_u64 needs a communicator (fk_comm_init*)");
    DeviceGuard dg_(c->device);
    std::string err;
    if (c->comm->allreduce_sum_u64(v, n, c->comm_stream, err)) return comm_fail(c, set_err(FK_E_COMM, "%s", err.c_str()));
    return FK_OK;
}

// ---- size-aware placement on the library's exchange (useCustomPartitioner, SBKC:1023-1026 and
// MultiprocessorSchedulingPartitioner.scala:35-69): every rank maps a sample of its input (no
// exchange), the per-bin k-mer totals are summed over the ranks (the reduceByKey of :1024), the
// LPT placement is computed identically on every rank and installed for the job's exchange.
static int sample_bin_kmers(fk_ctx *c, const uint8_t *sample, size_t n, std::vector<uint64_t> &sizes) {
    if (c->comm && c->job.xch.open) return set_err(FK_E_STATE, "bin placement inside a job's exchange");
    sizes.assign((size_t)c->Bc, 0);
    fk::Comm *comm = c->comm;
    c->comm = nullptr;  // the sample is mapped here, never exchanged
    int rc = n ? ingest_impl(c, sample, n, 1) : FK_OK;
    if (!rc && n) rc = map_records(c);
    if (!rc && n && c->nrec) {
        rc = part_count(c->binhist, map_src(c), 1, 1, nullptr, (uint32_t)c->Bc, c->ws, c->stream);
        if (!rc) {
            hipError_t e = hipMemcpyAsync(sizes.data(), c->binhist.kmer.p, (uint64_t)c->Bc * 8, hipMemcpyDeviceToHost,
                                          c->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
            if (e != hipSuccess) rc = set_err(FK_E_DEVICE, "sample histogram: %s", hipGetErrorString(e));
        }
    }
    c->comm = comm;
    c->ingest_fresh = true;
    c->mapped = false;
    c->have_result = false;
    return rc;
}

static int balance_from_sample(fk_ctx *c, const uint8_t *sample, size_t n) {
    DeviceGuard dg_(c->device);
    std::vector<uint64_t> sizes;
    FK_TRY(sample_bin_kmers(c, sample, n, sizes));
    if (c->comm) {
        std::string err;
        if (c->comm->allreduce_sum_u64(sizes.data(), sizes.size(), c->comm_stream, err))
            return set_err(FK_E_COMM, "bin size all-reduce: %s", err.c_str());
    }
    std::vector<int32_t> owner((size_t)c->Bc);
    FK_TRY(fk_lpt_owners(sizes.data(), c->Bc, (int32_t)c->G, owner.data()));
    return fk_set_bin_owners(c, owner.data(), nullptr);
}

FK_EXPORT int fk_balance_bins(fk_ctx *c, const uint8_t *sample, size_t n) {
    if (!c || (!sample && n)) return set_err(FK_E_INVALID, "null argument");
    const int rc = balance_from_sample(c, sample, n);
    return rc && c->comm ? comm_fail(c, rc) : rc;
}

// The sample of a file split: `fraction` of the rank's split as evenly spaced blocks of whole
// records (sequenceType 0) or of sequence (1, each block one record), the reference's
// sample(false, 0.01) of SBKC:1024 taken as blocks of the rank's own input.
static int split_sample(const char *path, int32_t world, int32_t rank, int32_t k, int32_t seq, double fraction,
                        std::vector<uint8_t> &out) {
    out.clear();
    Fd f;
    uint64_t size = 0;
    SplitPlan plan;
    FK_TRY(open_split(path, world, rank, k, seq, f, size, plan));
    if (plan.total == 0 || fraction <= 0.0) return FK_OK;
    std::vector<uint8_t> piece;
    std::string err;
    if (fraction >= 1.0) {
        out.resize(plan.total);
        if (read_split(f.fd, size, plan, 0, plan.total, out.data(), err)) return set_err(FK_E_IO, "%s", err.c_str());
        return FK_OK;
    }
    constexpr uint64_t BLOCK = 1ull << 20;
    const uint64_t want = std::max<uint64_t>((uint64_t)((double)plan.total * fraction), 1);
    const uint64_t nblk = std::max<uint64_t>(1, (want + BLOCK - 1) / BLOCK);
    const uint64_t blk = std::min<uint64_t>(plan.total, std::max<uint64_t>(4096, want / nblk));
    std::vector<uint8_t> buf;
    for (uint64_t i = 0; i < nblk; ++i) {
        const uint64_t at = plan.total * i / nblk, len = std::min(blk, plan.total - at);
        buf.resize(len);
        if (read_split(f.fd, size, plan, at, len, buf.data(), err)) return set_err(FK_E_IO, "%s", err.c_str());
        if (seq == 0) {  // whole records: from the first '>' opening a line to the last record start
            size_t a = 0;
            while (a < buf.size() && !(buf[a] == '>' && (a == 0 ? at == 0 : buf[a - 1] == '\n'))) ++a;
            size_t e = buf.size();
            if (at + len < plan.total) {
                while (e > a + 1 && !(buf[e - 1] == '>' && buf[e - 2] == '\n')) --e;
                e = e > a + 1 ? e - 1 : a;
            }
            out.insert(out.end(), buf.begin() + a, buf.begin() + e);
        } else {  // a block of the sequence as one record
            // the block's first line is dropped (it may be the tail of a header line: the block
            // started inside it, or the file's first header), and the block ends at the next
            // header line (a later record's name is not sequence)
            // -- unless the block holds no newline at all: it lies inside one sequence line (an unwrapped
            // record), and the whole block is sequence (a header line of a megabyte is not a FASTA)
            size_t a = 0;
            while (a < buf.size() && buf[a] != '\n') ++a;
            if (a == buf.size())
                a = (at == 0 && !buf.empty() && buf[0] == '>') ? buf.size() : 0;
            else
                a += 1;
            size_t e = a;
            while (e < buf.size() && !(buf[e] == '>' && e > 0 && buf[e - 1] == '\n')) ++e;
            if (e <= a) continue;
            const uint8_t h[3] = {'\n', '>', '\n'};
            out.insert(out.end(), h, h + 3);
            out.insert(out.end(), buf.begin() + a, buf.begin() + e);
        }
    }
    if (seq == 1) out.push_back('\n');
    if (seq == 1 && !out.empty()) out.erase(out.begin());  // the first block's header starts the input
    return FK_OK;
}

FK_EXPORT int fk_balance_bins_file(fk_ctx *c, const char *path, int32_t world, int32_t rank, double fraction) {
    if (!c || !path) return set_err(FK_E_INVALID, "null argument");
    if (c->in_format == FK_FORMAT_FASTQ)
        return set_err(FK_E_INVALID, "fk_balance_bins_file reads FASTA only: pass whole FASTQ records to fk_balance_bins");
    std::vector<uint8_t> sample;
    int rc = check_split_rank(c, world, rank, "fk_balance_bins_file");
    if (!rc) rc = split_sample(path, world, rank, c->cfg.k, c->cfg.sequence_type, fraction, sample);
    if (!rc) rc = balance_from_sample(c, sample.data(), sample.size());
    return rc && c->comm ? comm_fail(c, rc) : rc;
}

// Test hooks of the failure semantics (fastkmer.h): hold every stream the context's collectives run
// on with a kernel spinning on a host-mapped flag, so the next collective waits on a stream that does
// not drain; release it from any thread.
FK_EXPORT int fk_debug_comm_hold(fk_ctx *c, int32_t max_seconds) {
    if (!c || max_seconds < 1) return set_err(FK_E_INVALID, "bad argument");
    if (!c->comm) return set_err(FK_E_STATE, "fk_debug_comm_hold needs a communicator (fk_comm_init*)");
    DeviceGuard dg_(c->device);
    if (!c->hold_flag.p) HIP_TRY(c->hold_flag.alloc(64, hipHostMallocMapped | hipHostMallocCoherent));
    __atomic_store_n(c->hold_flag.as<uint32_t>(), 0u, __ATOMIC_RELEASE);
    void *dflag = nullptr;
    HIP_TRY(hipHostGetDevicePointer(&dflag, c->hold_flag.p, 0));
    // wall-clock ticks of max_seconds: the attribute is in kHz (100 MHz on gfx950); a rate reported
    // below that bounds the hold by 100 MHz ticks instead (longer, never shorter, than asked)
    int khz = 0;
    HIP_TRY(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->device));
    const uint64_t ticks = (uint64_t)max_seconds * (uint64_t)std::max(khz, 100000) * 1000ull;
    const hipStream_t cs2 = c->comm->counts_stream();
    for (hipStream_t st : {(hipStream_t)c->comm_stream, cs2})
        if (st) HIP_TRY(launch_hold_stream(static_cast<const uint32_t *>(dflag), ticks, st));
    return FK_OK;
}

FK_EXPORT int fk_debug_fingerprint_bits(int32_t device, int32_t bits) {
    DeviceGuard dg_(device);
    HIP_TRY(set_fingerprint_bits(bits));
    return FK_OK;
}

FK_EXPORT int fk_debug_comm_held(fk_ctx *c) {
    if (!c || !c->comm_stream) return 0;
    DeviceGuard dg_(c->device);
    const hipError_t e = hipStreamQuery(c->comm_stream);
    if (e != hipErrorNotReady) (void)hipGetLastError();
    return e == hipErrorNotReady ? 1 : 0;
}

FK_EXPORT int fk_debug_comm_release(fk_ctx *c) {
    if (!c) return set_err(FK_E_INVALID, "null ctx");
    if (c->hold_flag.p) __atomic_store_n(c->hold_flag.as<uint32_t>(), 1u, __ATOMIC_RELEASE);
    return FK_OK;
}

// ---------------------------------------------------------------------------
// test hook: one bucket through the wave tier (k_bucket_count64_wave / k_bucket_count128_wave)
// ---------------------------------------------------------------------------
// weighted: a 64-bit key may carry a weight field (bits [2k, 2k + 4), 2k <= WKEY_MAX_BITS)
static int debug_wave_count(int32_t device, int32_t k, int32_t F, uint32_t c0, uint32_t c1, int32_t slots,
                            const uint64_t *keys, uint32_t n, uint64_t *out_keys, uint32_t *out_counts,
                            uint32_t *n_out, bool weighted) {
    if (!keys || !out_keys || !out_counts || !n_out || k < 1 || k > 63 || F < 1 || F > MAX_FINE_BITS || c1 <= c0 ||
        c1 > (1u << F))
        return set_err(FK_E_INVALID, "bad argument");
    const int KW = k <= 32 ? 1 : 2;
    const uint32_t cap = KW == 1 ? WAVE_BUCKET_CAP : WAVE128_BUCKET_CAP;
    if (n == 0 || n > cap) return set_err(FK_E_RANGE, "a wave bucket holds 1..%u keys", cap);
    if (slots != (int32_t)(KW == 1 ? WAVE_SLOTS : 384))
        return set_err(FK_E_INVALID, "slots: %u (k <= 32) or 384 (k > 32)", WAVE_SLOTS);
    const int sh = 2 * k - F;
    for (uint32_t i = 0; i < n; ++i) {  // every key inside the bucket's cells
        const uint64_t hi = KW == 1 ? 0 : keys[2 * i];
        uint64_t lo = KW == 1 ? keys[i] : keys[2 * i + 1];
        if (weighted && KW == 1 && 2 * k <= WKEY_MAX_BITS && (lo >> (2 * k)) <= WKEY_WMAX - 1)
            lo &= (1ull << (2 * k)) - 1ull;  // the weight field; whatever else lies above the k-mer is refused below
        const uint64_t cell = sh >= 64 ? (hi >> (sh - 64)) : (sh == 0 ? lo : ((hi << (64 - sh)) | (lo >> sh)));
        if ((KW == 1 && k < 32 && (lo >> (2 * k)) != 0) || cell < c0 || cell >= c1)
            return set_err(FK_E_RANGE, "key %u lies outside cells [%u, %u)", i, c0, c1);
    }
    DeviceGuard dg_(device);
    DevBuf dk, dok, doc, du, db;
    FK_TRY(ensure(dk, (uint64_t)n * 8 * KW));
    FK_TRY(ensure(dok, (uint64_t)n * 8 * KW));
    FK_TRY(ensure(doc, (uint64_t)n * 4));
    FK_TRY(ensure(du, 16));
    FK_TRY(ensure(db, sizeof(Bucket)));
    const Bucket b{0, n, 0, c0, c1};
    BucketSrc wsrc{dk.as<uint64_t>(), F};
    wsrc.weighted = weighted;
    int rc = FK_OK;
    hipError_t e = hipMemcpy(dk.p, keys, (uint64_t)n * 8 * KW, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(db.p, &b, sizeof(Bucket), hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = KW == 1 ? launch_bucket_count64_wave(wsrc, db.as<Bucket>(), 1, k, dok.as<uint64_t>(),
                                                 doc.as<uint32_t>(), du.as<uint64_t>(), nullptr, nullptr)
                    : launch_bucket_count128_wave(BucketSrc{dk.as<uint64_t>(), F}, db.as<Bucket>(), 1, k, dok.as<uint64_t>(),
                                                  doc.as<uint32_t>(), du.as<uint64_t>(), nullptr);
    uint64_t U = 0;
    if (e == hipSuccess) e = hipMemcpy(&U, du.p, 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess && U <= n) e = hipMemcpy(out_keys, dok.p, U * 8 * KW, hipMemcpyDeviceToHost);
    if (e == hipSuccess && U <= n) e = hipMemcpy(out_counts, doc.p, U * 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) rc = set_err(FK_E_DEVICE, "%s", hipGetErrorString(e));
    else if (U > n) rc = set_err(FK_E_INVALID, "bucket reported %llu distinct keys of %u", (unsigned long long)U, n);
    *n_out = (uint32_t)U;
    return rc;
}

FK_EXPORT int fk_debug_wave_count(int32_t device, int32_t k, int32_t F, uint32_t c0, uint32_t c1, int32_t slots,
                                  const uint64_t *keys, uint32_t n, uint64_t *out_keys, uint32_t *out_counts,
                                  uint32_t *n_out) {
    return debug_wave_count(device, k, F, c0, c1, slots, keys, n, out_keys, out_counts, n_out, false);
}

FK_EXPORT int fk_debug_wave_count_w(int32_t device, int32_t k, int32_t F, uint32_t c0, uint32_t c1, int32_t slots,
                                    const uint64_t *keys, uint32_t n, uint64_t *out_keys, uint32_t *out_counts,
                                    uint32_t *n_out) {
    return debug_wave_count(device, k, F, c0, c1, slots, keys, n, out_keys, out_counts, n_out, true);
}

FK_EXPORT int fk_debug_fold_stats(const fk_ctx *c, uint64_t out[4]) {
    if (!c || !out) return set_err(FK_E_INVALID, "null argument");
    std::copy(c->fold_last, c->fold_last + 4, out);
    return FK_OK;
}

// ---------------------------------------------------------------------------
// test hooks: the staged count (the bucket cut, every tier, the fold) over caller-supplied pieces
// ---------------------------------------------------------------------------
// Nothing of the count is reimplemented: the context is filled the way staged_expand_chunks fills it
// (st_keys, st_cb, st_total, st_plan, st_np, st_kmers), then fold_piece and staged_count run as they
// do in a job, and the context is left as fk_finish leaves it.
FK_EXPORT int fk_debug_count_pieces(fk_ctx *c, int32_t F, int32_t np, const uint64_t *const *keys,
                                    const uint64_t *const *cell_counts, int32_t weighted, uint32_t fold_mask) {
    if (!c || !keys || !cell_counts) return set_err(FK_E_INVALID, "null argument");
    const int k = c->cfg.k, KW = c->KW;
    if (!staged_eligible(c)) return set_err(FK_E_INVALID, "staged pieces need k <= 63, one rank and no communicator");
    if (c->job.job_open) return set_err(FK_E_STATE, "fk_debug_count_pieces inside a job (after its first fk_ingest)");
    if (F < 1 || F > std::min(MAX_FINE_BITS, 2 * k)) return set_err(FK_E_INVALID, "F = %d outside 1 .. min(%d, 2k)", F, MAX_FINE_BITS);
    if (np < 1 || (uint32_t)np > stage_maxp(c)) return set_err(FK_E_INVALID, "%d pieces: 1 .. %u", np, stage_maxp(c));
    const bool wfield = KW == 1 && 2 * k <= WKEY_MAX_BITS;
    if ((weighted || fold_mask) && !wfield)
        return set_err(FK_E_INVALID, "k = %d: no weight field (weighted keys and the fold need 2k <= %d)", k, WKEY_MAX_BITS);
    if (fold_mask >> np) return set_err(FK_E_INVALID, "fold_mask names a piece past the %d given", np);
    for (int p = 0; p < np; ++p)
        if (!keys[p] || !cell_counts[p]) return set_err(FK_E_INVALID, "null piece %d", p);
    // every key in the cell and bin its position says, nothing above the k-mer but a weight, no EMPTY_KEY
    // (~0: at k = 30 the all-T k-mer under weight 15 -- canonical k-mers are never all T, and the weight
    // field stops at 14 + 1)
    const uint32_t nlb = c->nlb;
    const uint64_t ncell_all = (uint64_t)nlb << F;
    const int sh = 2 * k - F;
    std::vector<std::vector<uint64_t>> cb((size_t)np);
    std::vector<uint64_t> total(ncell_all, 0);
    uint64_t sumw = 0, entries = 0;
    for (int p = 0; p < np; ++p) {
        uint64_t maxw = 1;
        cb[p].assign(ncell_all + 1, 0);
        for (uint64_t g = 0; g < ncell_all; ++g) {
            const uint64_t n = cell_counts[p][g];
            if (n >= (1ull << 32)) return set_err(FK_E_RANGE, "piece %d, cell %llu: %llu keys", p, (unsigned long long)g, (unsigned long long)n);
            cb[p][g + 1] = cb[p][g] + n;
            total[g] += n;
            const int32_t bin = global_bin(c, (uint32_t)(g >> F));
            const uint64_t cell = g & ((1ull << F) - 1);
            for (uint64_t i = cb[p][g]; i < cb[p][g + 1]; ++i) {
                KmerKey f = KW == 1 ? KmerKey{0, keys[p][i]} : KmerKey{keys[p][2 * i], keys[p][2 * i + 1]};
                uint64_t w = 1;
                if (KW == 1 && f.lo == ~0ull) return set_err(FK_E_RANGE, "piece %d, key %llu is EMPTY_KEY", p, (unsigned long long)i);
                if (weighted) {
                    w += f.lo >> (2 * k);
                    if (w > WKEY_WMAX) return set_err(FK_E_RANGE, "piece %d, key %llu: bits above the weight field", p, (unsigned long long)i);
                    f.lo &= (1ull << (2 * k)) - 1ull;
                }
                if (!key_is_kmer(f, k)) return set_err(FK_E_RANGE, "piece %d, key %llu: bits above the k-mer", p, (unsigned long long)i);
                const uint64_t kc = sh >= 64 ? (f.hi >> (sh - 64)) : (sh == 0 ? f.lo : ((KW == 2 ? f.hi << (64 - sh) : 0ull) | (f.lo >> sh)));
                if (kc != cell) return set_err(FK_E_RANGE, "piece %d, key %llu lies in cell %llu, not %llu", p, (unsigned long long)i, (unsigned long long)kc, (unsigned long long)cell);
                const uint32_t sig = KW == 2 ? kmer_signature<true>(f, revcomp_key<true>(f, k), k, c->cfg.m)
                                             : kmer_signature<false>(f, revcomp_key<false>(f, k), k, c->cfg.m);
                if ((int32_t)bin_of_signature(sig, c->fm) != bin)
                    return set_err(FK_E_RANGE, "piece %d, key %llu belongs to bin %d, not %d", p, (unsigned long long)i, (int32_t)bin_of_signature(sig, c->fm), bin);
                sumw += w;
                maxw = std::max(maxw, w);
            }
        }
        // a k-mer of multiplicity m folds to ceil(m / wmax) entries: at most the piece's keys (the room the
        // fold has, as in a job, whose pieces arrive unweighted) only while no weight exceeds wmax
        if ((fold_mask >> p & 1u) && maxw > c->fold_wmax)
            return set_err(FK_E_INVALID, "piece %d holds weight %llu above the fold's cap %u: the fold would grow it", p,
                           (unsigned long long)maxw, c->fold_wmax);
        entries += cb[p][ncell_all];
    }
    if (entries == 0) return set_err(FK_E_INVALID, "no keys");
    DeviceGuard dg_(c->device);
    const StreamWs on = c->main_on();
    hipStream_t s = on.s;
    HIP_TRY(hipStreamSynchronize(s));
    // pieces without an input (no job is open, see above): a new result over staged pieces of their own;
    // the last input and what fk_map or fk_debug_fastq_ms would read of its job stay
    end_pieces(c);
    new_result(c);
    c->nkmers = sumw;
    c->stats.kmers = sumw;
    c->job.st_plan = sorted_plan(c, entries, F);
    if (!c->job.st_plan.tiered || !c->job.st_plan.two_level) return set_err(FK_E_STATE, "staged pieces need the tiered two-level count");
    uint64_t maxp = 0;
    for (int p = 0; p < np; ++p) {
        const uint64_t n = cb[p][ncell_all];
        maxp = std::max(maxp, n);
        FK_TRY(ensure(c->st_keys[p], std::max<uint64_t>(n, 1) * 8 * KW));
        FK_TRY(ensure(c->st_cb[p], (ncell_all + 1) * 8));
        if (n) HIP_TRY(hipMemcpy(c->st_keys[p].p, keys[p], n * 8 * KW, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(c->st_cb[p].p, cb[p].data(), (ncell_all + 1) * 8, hipMemcpyHostToDevice));
    }
    FK_TRY(ensure(c->st_total, ncell_all * 8));
    HIP_TRY(hipMemcpy(c->st_total.p, total.data(), ncell_all * 8, hipMemcpyHostToDevice));
    c->job.st_np = (uint32_t)np;
    c->job.st_kmers = entries;
    c->job.st_weighted = weighted != 0;
    int rc = FK_OK;
    if (fold_mask) rc = ensure(c->mid, maxp * 8);  // the fold's scratch: in a job, the piece's first expansion level
    for (int p = 0; p < np && rc == FK_OK; ++p)
        if (fold_mask >> p & 1u) rc = fold_piece(c, on, (uint32_t)p, cb[p][ncell_all]);
    if (rc == FK_OK) rc = staged_count(c, nullptr);
    if (rc == FK_OK) fold_report(c, true);
    end_pieces(c);
    return rc;
}

FK_EXPORT int fk_debug_tier_stats(const fk_ctx *c, uint64_t out[8]) {
    if (!c || !out) return set_err(FK_E_INVALID, "null argument");
    std::copy(c->tier_last, c->tier_last + 8, out);
    return FK_OK;
}

FK_EXPORT int fk_debug_live_resources(uint64_t out[4]) {
    if (!out) return set_err(FK_E_INVALID, "null argument");
    for (int i = 0; i < 4; ++i) out[i] = g_live[i].load(std::memory_order_relaxed);
    return FK_OK;
}

FK_EXPORT int fk_debug_staged_piece(fk_ctx *c, int32_t p, uint64_t *out_keys, uint64_t *out_cb) {
    if (!c || !out_cb) return set_err(FK_E_INVALID, "null argument");
    if (!c->have_result || p < 0 || (uint32_t)p >= c->last_np)
        return set_err(FK_E_STATE, "piece %d: the last job counted %u staged pieces", p, c->have_result ? c->last_np : 0u);
    DeviceGuard dg_(c->device);
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(out_cb, c->st_cb[p].p, (c->last_cells + 1) * 8, hipMemcpyDeviceToHost));
    const uint64_t n = out_cb[c->last_cells];
    if (out_keys && n) HIP_TRY(hipMemcpy(out_keys, c->st_keys[p].p, n * 8 * c->KW, hipMemcpyDeviceToHost));
    return FK_OK;
}

// measurement hook (a library built with -DFK_PROBES; FK_E_STATE otherwise): the fused map's
// per-phase wave cycles (s_memtime) summed over every launch since the last reset
FK_EXPORT int fk_debug_map_cycles(uint64_t *out16, int32_t reset) {
    if (!out16) return set_err(FK_E_INVALID, "null argument");
    const hipError_t e = map_fused_cycles(reinterpret_cast<unsigned long long *>(out16), reset != 0);
    if (e == hipErrorNotSupported) {
        (void)hipGetLastError();
        return set_err(FK_E_STATE, "phase stamps exist only in a library built with -DFK_PROBES");
    }
    HIP_TRY(e);
    return FK_OK;
}

FK_EXPORT int fk_get_stats(fk_ctx *c, fk_stats *out) {
    if (!c || !out) return set_err(FK_E_INVALID, "null argument");
    *out = c->stats;
    return FK_OK;
}

// ---------------------------------------------------------------------------
// bin-signature diagnostics (executeFindBinSignaturesJob, SBKC:956-986)
// ---------------------------------------------------------------------------

FK_EXPORT uint64_t fk_signature_slots(const fk_ctx *c) { return c ? (1ull << (2 * c->cfg.m)) + 1ull : 0ull; }

// getBinSignatures (SBKC:772-917) over the ingested input: the FASTA parse
// (fk_parse.inc, look-back variant) and one pass of k_bin_signatures.  The
// input stays as it was, so fk_map may follow.
FK_EXPORT int fk_signature_counts(fk_ctx *c, void *d_counts, uint64_t n_counts) {
    if (!c || !d_counts) return set_err(FK_E_INVALID, "null argument");
    DeviceGuard dg_(c->device);
    const uint64_t slots = fk_signature_slots(c);
    if (n_counts < slots)
        return set_err(FK_E_RANGE, "signature counts hold %llu entries, need 4^m + 1 = %llu",
                       (unsigned long long)n_counts, (unsigned long long)slots);
    if (c->job.pm_active && !c->job.pm_last_seen)
        return set_err(FK_E_STATE, "fk_signature_counts inside a streamed input: finish it with fk_ingest(..., last = 1)");
    hipStream_t s = c->stream;
    const uint64_t n = c->d_fasta ? c->n_fasta : 0;
    HIP_TRY(hipMemsetAsync(d_counts, 0, slots * 8, s));
    FK_TRY(fq_finish_pending(c, n));  // FASTQ: the input ends here (fk_map reports a malformed record)
    if (n) {
        const uint64_t ntiles = (n + ENC_TILE - 1) / ENC_TILE;
        const uint64_t code_words = n / 16 + 2 * POS_PAD_WORDS + 512;
        const uint64_t valid_words = n / 32 + 2 * POS_PAD_WORDS + 512;
        FK_TRY(ensure(c->tile_last_nl, ntiles * 8));
        FK_TRY(ensure(c->tile_off, ntiles * 8));
        FK_TRY(ensure(c->npos_dev, 16));
        FK_TRY(ensure(c->codes, code_words * 4));
        FK_TRY(ensure(c->valid, valid_words * 4));
        HIP_TRY(hipMemsetAsync(c->codes.p, 0, code_words * 4, s));
        HIP_TRY(hipMemsetAsync(c->valid.p, 0, valid_words * 4, s));
        HIP_TRY(hipMemsetAsync(c->npos_dev.p, 0, 16, s));
        HIP_TRY(hipMemsetAsync(c->tile_last_nl.p, 0, ntiles * 8, s));
        HIP_TRY(hipMemsetAsync(c->tile_off.p, 0, ntiles * 8, s));
        HIP_TRY(launch_fasta_parse(false, c->d_fasta, n, c->tile_last_nl.as<uint64_t>(), c->tile_off.as<uint64_t>(),
                                   c->codes.as<uint32_t>(), c->valid.as<uint32_t>(), c->npos_dev.as<uint64_t>(), s));
        HIP_TRY(launch_bin_signatures(c->codes.as<uint32_t>(), c->valid.as<uint32_t>(), n, c->npos_dev.as<uint64_t>(),
                                      c->cfg.k, c->cfg.m, (unsigned long long *)d_counts, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    return FK_OK;
}

// longToString (PKG:616-634): always nucleotidesPerLong = 31 characters, the
// signature's base-4 digits right-aligned behind 'A's (its length argument is unused).
static void signature_string(uint64_t v, char out[31]) {
    static const char rep[4] = {'A', 'C', 'G', 'T'};
    for (int j = 30; j >= 0; --j) {
        out[j] = rep[v & 3u];
        v >>= 2;
    }
}

// saveBinSignatures (SBKC:920-953): <out_dir>/bin_signatures<b>.txt for every
// bin this rank owns that holds a signature, "<signature>\t<count>\n" lines
// (ascending signature; the reference iterates a HashMap) and "Total\t<sum>\n".
FK_EXPORT int fk_write_bin_signatures(fk_ctx *c, const void *d_counts, uint64_t n_counts, const char *out_dir) {
    if (!c || !d_counts || !out_dir) return set_err(FK_E_INVALID, "null argument");
    DeviceGuard dg_(c->device);
    const uint64_t slots = fk_signature_slots(c);
    if (n_counts < slots)
        return set_err(FK_E_RANGE, "signature counts hold %llu entries, need 4^m + 1 = %llu",
                       (unsigned long long)n_counts, (unsigned long long)slots);
    hipStream_t s = c->stream;
    const unsigned long long *counts = (const unsigned long long *)d_counts;
    DevBuf nz, pairs;
    FK_TRY(ensure(nz, 8));
    unsigned long long nnz = 0;
    HIP_TRY(hipMemsetAsync(nz.p, 0, 8, s));
    HIP_TRY(launch_sig_compact(counts, slots, nullptr, nz.as<unsigned long long>(), s));
    HIP_TRY(hipMemcpyAsync(&nnz, nz.p, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    std::vector<uint64_t> h(2 * nnz);
    if (nnz) {
        FK_TRY(ensure(pairs, nnz * 16));
        HIP_TRY(hipMemsetAsync(nz.p, 0, 8, s));
        HIP_TRY(launch_sig_compact(counts, slots, pairs.as<uint64_t>(), nz.as<unsigned long long>(), s));
        HIP_TRY(hipMemcpyAsync(h.data(), pairs.p, nnz * 16, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    // (bin, signature) order; bins owned by other ranks are theirs to write
    std::vector<std::pair<uint64_t, uint64_t>> rows;  // (bin << 32 | signature, count)
    rows.reserve(nnz);
    for (uint64_t i = 0; i < nnz; ++i) {
        const uint32_t sig = (uint32_t)h[2 * i];
        const int32_t b = (int32_t)bin_of_signature(sig, c->fm);
        if (owns(c, b)) rows.emplace_back(((uint64_t)b << 32) | sig, h[2 * i + 1]);
    }
    std::sort(rows.begin(), rows.end());
    if (rows.empty()) return FK_OK;
    if (mkdir_p(out_dir) != 0) return set_err(FK_E_IO, "cannot create %s: %s", out_dir, strerror(errno));
    const std::string dir(out_dir);
    std::string text;
    for (size_t i = 0; i < rows.size();) {
        const uint32_t b = (uint32_t)(rows[i].first >> 32);
        uint64_t tot = 0;
        text.clear();
        for (; i < rows.size() && (uint32_t)(rows[i].first >> 32) == b; ++i) {
            char sig[31];
            signature_string((uint32_t)rows[i].first, sig);
            text.append(sig, 31);
            text.push_back('\t');
            text += std::to_string(rows[i].second);
            text.push_back('\n');
            tot += rows[i].second;
        }
        text += "Total\t" + std::to_string(tot) + "\n";
        const std::string path = dir + "/bin_signatures" + std::to_string(b) + ".txt";
        FILE *f = fopen(path.c_str(), "wb");
        const bool ok = f && fwrite(text.data(), 1, text.size(), f) == text.size();
        if (f && fclose(f) != 0) return set_err(FK_E_IO, "closing %s failed", path.c_str());
        if (!ok) return set_err(FK_E_IO, "writing %s failed", path.c_str());
    }
    return FK_OK;
}

// executeFindBinSignaturesJob (SBKC:956-986) for one rank holding the whole
// input: fk_signature_counts into a context-owned buffer, then the writer.
FK_EXPORT int fk_find_bin_signatures(fk_ctx *c, const char *out_dir) {
    if (!c || !out_dir) return set_err(FK_E_INVALID, "null argument");
    DeviceGuard dg_(c->device);
    const uint64_t slots = fk_signature_slots(c);
    DevBuf counts;
    FK_TRY(ensure(counts, slots * 8));
    FK_TRY(fk_signature_counts(c, counts.p, slots));
    return fk_write_bin_signatures(c, counts.p, slots, out_dir);
}
