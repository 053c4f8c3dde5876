// fk_ctx.h -- private: the context behind the C-ABI's fk_ctx and the host helpers shared by fk_api.cpp (the
// context, the input and the count), fk_views.cpp (the calls that only read a finished result) and fk_store.cpp
// (export, import and the database file).  All are compiled with the same -D flags (fk_ctx has FK_PROBES members).
//
// First the owner types of the GPU handles (PinBuf, DevBuf, Event, Stream; ScanWorkspace is in
// fk_internal.h): move-only, freed by their destructors, counted for fk_debug_live_resources.  Then
// fk_ctx, its members sorted by lifetime: fixed at fk_create / as long as the context / settings of the
// next job / the job in flight (fk_ctx::Job, begun by begin_job alone) / the last map and result.
// DESIGN.md, "The context: what lives how long", has the stream and event roles.
#pragma once

#include <algorithm>
#include <atomic>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/fastkmer.h"
#include "fk_comm.h"
#include "fk_internal.h"

#define FK_EXPORT extern "C" __attribute__((visibility("default")))

namespace fk {
int set_err(int code, const char *fmt, ...);  // fk_api.cpp: the calling thread's fk_last_error message; returns code
int mkdir_p(const std::string &path);         // fk_views.cpp
// what the lookups, the comparison's kin and the export / import answer on a use_ht = 1 context
constexpr const char *MSG_NEED_SORTED = "lookups need the sorted count (use_ht = 0): a use_ht = 1 result is in table order";

#define HIP_TRY(expr)                                                                                \
    do {                                                                                             \
        hipError_t e_ = (expr);                                                                      \
        if (e_ != hipSuccess)                                                                        \
            return set_err(e_ == hipErrorOutOfMemory ? FK_E_NOMEM : FK_E_DEVICE, "%s failed: %s (%s:%d)", \
                           #expr, hipGetErrorString(e_), __FILE__, __LINE__);                        \
    } while (0)

#define FK_TRY(expr)             \
    do {                         \
        int r_ = (expr);         \
        if (r_ != FK_OK) return r_; \
    } while (0)

// ---- owners of the GPU handles.  Each is move-only and frees what it holds when it dies, so a struct
// of them (fk_ctx, PartBufs, ViewBufs, a call's locals) needs no release list.  Whoever destroys one
// has drained the streams that use it (fk_destroy; a call's temporaries: the call itself).
// fk_debug_live_resources counts what they hold, process-wide.
enum { LIVE_DEV, LIVE_PIN, LIVE_EVENT, LIVE_STREAM };
inline std::atomic<uint64_t> g_live[4];
inline void live(int what, int64_t d) { g_live[what].fetch_add((uint64_t)d, std::memory_order_relaxed); }

// Pinned host memory, grow-only: small uploads and read-backs on the hot path go
// through it (pageable transfers are staged by the runtime, and block the host).
struct PinBuf {
    void *p = nullptr;
    size_t bytes = 0;
    PinBuf() = default;
    PinBuf(PinBuf &&o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr, o.bytes = 0; }
    PinBuf &operator=(PinBuf &&o) noexcept {
        if (this != &o) release(), p = o.p, bytes = o.bytes, o.p = nullptr, o.bytes = 0;
        return *this;
    }
    ~PinBuf() { release(); }
    // exactly `want` bytes with hipHostMalloc's flags (a mapped flag word, a staging buffer of a fixed size)
    hipError_t alloc(size_t want, unsigned flags) {
        release();
        const hipError_t e = hipHostMalloc(&p, want, flags);
        if (e != hipSuccess) return p = nullptr, e;
        live(LIVE_PIN, 1);
        bytes = want;
        return hipSuccess;
    }
    int ensure(size_t need) {
        if (bytes >= need) return FK_OK;
        if (alloc(std::max<size_t>(need + need / 4, 4096), hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            return FK_E_NOMEM;
        }
        return FK_OK;
    }
    void release() {
        if (p) (void)hipHostFree(p), live(LIVE_PIN, -1);
        p = nullptr;
        bytes = 0;
    }
    template <typename T>
    T *as() const { return reinterpret_cast<T *>(p); }
};

// Device memory, grow-only (ensure); a call's own temporary is a local one, and the call drains the
// stream that reads it before it returns.
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr, o.bytes = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) release(), p = o.p, bytes = o.bytes, o.p = nullptr, o.bytes = 0;
        return *this;
    }
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p), live(LIVE_DEV, -1);
        p = nullptr;
        bytes = 0;
    }
    template <typename T>
    T *as() const { return reinterpret_cast<T *>(p); }
};

inline void release(DevBuf &b) { b.release(); }

inline int ensure(DevBuf &b, size_t bytes) {
    if (bytes == 0) bytes = 16;
    if (b.bytes >= bytes) return FK_OK;
    b.release();
    // slack for the next job's slightly larger input: an eighth, at most 1 GiB (4 GB of slack on each
    // k-mer array of a 6.25 GB job would cost more HBM than the reallocations it saves)
    const size_t want = bytes + std::min<size_t>(bytes / 8, 1ull << 30) + 256;
    hipError_t e = hipMalloc(&b.p, want);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        b.p = nullptr;
        return set_err(FK_E_NOMEM, "hipMalloc(%zu) failed: %s", want, hipGetErrorString(e));
    }
    live(LIVE_DEV, 1);
    b.bytes = want;
    return FK_OK;
}

// An event; converts to its handle (null until create).
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(Event &&o) noexcept : e(o.e) { o.e = nullptr; }
    Event &operator=(Event &&o) noexcept {
        if (this != &o) destroy(), e = o.e, o.e = nullptr;
        return *this;
    }
    ~Event() { destroy(); }
    hipError_t create(unsigned flags = hipEventDefault) {  // timed by default; kept if it exists
        if (e) return hipSuccess;
        const hipError_t r = hipEventCreateWithFlags(&e, flags);
        if (r != hipSuccess) return e = nullptr, r;
        live(LIVE_EVENT, 1);
        return hipSuccess;
    }
    void destroy() {
        if (e) (void)hipEventDestroy(e), live(LIVE_EVENT, -1);
        e = nullptr;
    }
    operator hipEvent_t() const { return e; }
};

// Grows v to at least n events created with `flags` (the lazily grown per-segment / per-step events).
inline hipError_t ensure_events(std::vector<Event> &v, size_t n, unsigned flags = hipEventDefault) {
    while (v.size() < n) {
        Event e;
        const hipError_t r = e.create(flags);
        if (r != hipSuccess) return r;
        v.push_back(std::move(e));
    }
    return hipSuccess;
}

// A non-blocking stream the context created, or one it borrows (fk_set_stream: never destroyed);
// converts to its handle.
struct Stream {
    hipStream_t s = nullptr;
    bool own = false;
    Stream() = default;
    Stream(Stream &&o) noexcept : s(o.s), own(o.own) { o.s = nullptr, o.own = false; }
    Stream &operator=(Stream &&o) noexcept {
        if (this != &o) destroy(), s = o.s, own = o.own, o.s = nullptr, o.own = false;
        return *this;
    }
    ~Stream() { destroy(); }
    hipError_t create(const int *priority = nullptr) {  // kept if it exists
        if (s) return hipSuccess;
        const hipError_t r = priority ? hipStreamCreateWithPriority(&s, hipStreamNonBlocking, *priority)
                                      : hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
        if (r != hipSuccess) return s = nullptr, r;
        live(LIVE_STREAM, 1);
        own = true;
        return hipSuccess;
    }
    void borrow(hipStream_t other) {
        destroy();
        s = other;
    }
    void destroy() {
        if (s && own) (void)hipStreamDestroy(s), live(LIVE_STREAM, -1);
        s = nullptr;
        own = false;
    }
    operator hipStream_t() const { return s; }
};

template <typename T>
constexpr bool move_only = !std::is_copy_constructible_v<T> && !std::is_copy_assignable_v<T> &&
                           std::is_nothrow_move_constructible_v<T> && std::is_nothrow_move_assignable_v<T>;
static_assert(move_only<PinBuf> && move_only<DevBuf> && move_only<Event> && move_only<Stream> && move_only<ScanWorkspace>,
              "an owner of a GPU handle has one holder");

// Record partition (fk_partition.inc): histogram -> scan -> scatter.
struct PartBufs {
    DevBuf H, K, Hs, Ts, KT;              // per-workgroup histograms and destinations (rows), segment sums
    DevBuf rec, kmer, off, cursor;        // per-part totals / offsets (device), cursor: global path only
    uint32_t nparts = 0;
    RecSrc src{};                         // the records counted (part_scatter reads the same)
    bool global = false;                  // nparts > PART_MAX: global-atomic kernels
};

inline int32_t clamp_bins(int32_t m, int32_t B) {
    // test/package.scala:32: Math.min(Math.pow(4, m), max_b).toInt
    double p = 1.0;
    for (int i = 0; i < m; ++i) p *= 4.0;
    const double b = p < (double)B ? p : (double)B;
    return (int32_t)b;
}

// Every exported call that touches the GPU selects the context's device for
// its duration and restores the caller's current device on return, so one
// thread may drive contexts on several GPUs and a context may move between
// threads (e.g. JNI executor threads).
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) {
            (void)hipGetLastError();
            prev = -1;
        }
        if (dev >= 0 && prev != dev) {
            (void)hipSetDevice(dev);
        } else {
            prev = -1;  // nothing to restore
        }
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};

// The sorted count's shape: cell bits F (super-cells of 2^F2 cells), tiers.
struct SortedPlan {
    int F = 1, F2 = 0, F1 = 1;
    bool tiered = false, two_level = false;
    uint32_t cap = 2048, wave_cap = WAVE_BUCKET_CAP;
    uint64_t max_bin = 0;  // the largest bin's k-mers the plan was made for
};

// A stream and the scan workspace its scans use.  The count's stages take one as a parameter: the
// context's own (`stream`, `ws`) or the staging stream's (`xstage`, `ws_x`); see main_on / stage_on.
// A scan owns its workspace from launch to completion, so two streams share one only while their
// scans are ordered by events.  The side stream (`tier_side`) borrows the main stream's workspace
// under this rule: its scans (the last piece's bucket cut, the split's sizes) are queued behind a wait
// for an event recorded on the main stream after that stream's last scan (side_ev[2] after the
// cell-offset scan of the last piece, or side_ev[3] behind the cut), and the main stream queues no scan
// again until it has waited for the side stream's work (side_ev[0] after the cut, side_ev[1] after the
// heavy tiers: the result's scans follow it).
struct StreamWs {
    hipStream_t s;
    ScanWorkspace *ws;
};

// The result views' staging (fk_views.cpp): grow-only, reused from call to call.
struct ViewBufs {
    DevBuf gather_keys, gather_counts, gather_other;  // one bin gathered or filtered (other: its counts in the other result)
    DevBuf q_in, q_counts, q_bins;      // fk_query / fk_query_sequence: one chunk's keys (or bases), counts and bins
    DevBuf rd_off, rd_valid, rd_stats;  // fk_read_counts / _stats: one chunk's offsets, valid flags, statistics (bases in q_in)
    DevBuf sp_hist, cmp_mat;            // fk_spectrum: the histogram and its tail sum; fk_compare: the matrix
    DevBuf rg_kept, rg_off;             // a filtered bin: kept k-mers per bucket of the bin and their scan
};

}  // namespace fk
using namespace fk;

// The context.  Its members are sorted by how long they live ("The context: what lives how long").
// A device handle in it is an owner type: fk_destroy drains the streams and deletes the context, it names
// no member.
struct fk_ctx {
    // ---- 1. fixed at fk_create: the configuration and what follows from it, the environment's sizes,
    // cuts and test hooks
    fk_config cfg{};
    int32_t Bc = 0;    // b = min(4^m, B)
    uint32_t G = 1;    // ranks
    uint32_t nlb = 0;  // local bins: b = rank + G * lb (default placement) or lbin_bin[lb] (custom)
    int W = 2, KW = 1;
    FastMod fm{};
    int device = 0;
    uint64_t piece_bytes = 512ull << 20;         // FASTKMER_PIECE_BYTES: FASTA bytes per piece (with a
                                                 // communicator: a tenth of a known job, 128 MB .. 1 GB)
    bool piece_bytes_set = false;
    uint64_t ingest_seg = 32ull << 20;           // FASTKMER_INGEST_SEG: H2D segment of a pinned source
    std::vector<double> st_cuts{0.4, 0.7, 0.9};  // piece ends of a staged job (FASTKMER_PIECE_CUTS; 45 / 70 / 85 % measured 22.84 vs 22.77 ms)
    // ... of a 64-bit job of >= 4 GB without FASTKMER_PIECE_CUTS: five pieces, the last 7 % (configs[2]
    // load 146.2 -> 145.4 ms, profiles/r06z_five_pieces.txt; configs[1]'s 1 GB keeps four)
    std::vector<double> st_cuts5{0.38, 0.64, 0.82, 0.93};
    bool cuts_env = false;
    // ... with a communicator: earlier, a received piece lands a step's partition and transfer later
    // (one in-process rank at the configs[2] load: 153.2-153.7 ms against 156.1-159.4 with the local
    // cuts, profiles/r05z_xch_cuts_seg_ab.txt)
    std::vector<double> xst_cuts{0.35, 0.65, 0.84};
    int fold_mode = 1;                           // FASTKMER_FOLD: 0 off, 1 by the first piece's sample, 2 every eligible piece
    int x2_l1 = 0;             // FASTKMER_X2_L1: level-1 workgroup size (512, 1024; 0 = by fan-out)
    int fused = 1;             // FASTKMER_FUSED=0: two-kernel map (parse, then signature) for every input
    // Test hooks (result-preserving; they steer inputs that FASTA data cannot aim at onto a path):
    bool force_large = false;  // FASTKMER_DEBUG_LARGE_BUCKETS=1: route every bucket through the streaming path
    uint32_t cell_target = 0;  // FASTKMER_DEBUG_CELL_TARGET: average keys per cell of the largest bin (0: auto)
    int mid_parts = -1;        // FASTKMER_DEBUG_MID_PARTS: the 64-bit mid tier's key ranges always (1), the whole
                               // buckets on the 512-key table always (2), the 1024-key kernel only (0), by size (-1)
    bool split_retry = false;  // FASTKMER_DEBUG_SPLIT_RETRY: every split bucket cut a second time
    bool spectrum_wide = false;  // FASTKMER_DEBUG_SPECTRUM_WIDE: the spectrum kernel of results of >= 2^32 k-mers
    uint32_t import_bucket = 0;  // FASTKMER_DEBUG_IMPORT_BUCKET=<keys>: an imported result's buckets are cut at this
                                 // many keys (0: the wave tier's capacity); read by every fk_import* / fk_load
    uint32_t fold_wmax = WKEY_WMAX;              // FASTKMER_DEBUG_FOLD_WMAX: a lower weight cap (test hook)
#ifdef FK_PROBES
    // Measurement-only (a library built with -DFK_PROBES; wrong results by design):
    int dbg_phase = 99;        // FASTKMER_DEBUG_PHASE: stop the bucket kernel early
    int fused_probe = 0;       // FASTKMER_FUSED_PROBE: stop the fused map kernel after a phase
    int split_map = 0;         // FASTKMER_SPLIT_MAP=1: the map as a parse kernel + a signature-pass kernel
#endif

    // ---- 2. as long as the context: streams, events, buffers and workspaces, grow-only, each an owner.
    // Streams (their roles and the events between them: DESIGN.md):
    Stream stream;       // the map and the count; the caller's after fk_set_stream (borrowed)
    Stream copy_stream;  // H2D of fk_ingest (the map runs on `stream` meanwhile)
    Stream xstage;       // staged pieces / received segments partitioned and expanded, with its own workspace ws_x
    Stream tier_side;    // the count's heavy tiers beside the wave tier, the last piece's cut (highest priority)
    Stream comm_stream;  // the exchange's transfers (with a communicator)
    fk::Comm *comm = nullptr;
    ScanWorkspace ws, ws_x;
    StreamWs main_on() { return StreamWs{stream, &ws}; }
    StreamWs stage_on() { return StreamWs{xstage, &ws_x}; }
    // Events; timed: ev, st_ev, h2d_ev, fq_evs, xev, the rest order streams only (hipEventDisableTiming)
    Event ev[12];                // 0/1 parse, 2/3 signature, 4/5 partition, 6/7 count, 8/9 encode kernel, 10/11 sig kernel
    Event st_ev[4 * STAGE_MAXP]; // per piece: partition begin / end, expansion begin / end
    Event side_ev[4];            // [0] cut -> wave tier, [1] heavy tiers -> result, [2] last piece's cell offsets -> cut, [3] -> heavy
    Event h2d_ev[2];             // first copy issued / last copy done
    Event pin_ev[2];             // pinned[i]'s DMA is done
    Event seg_ev;                // "segment landed" (copy stream -> map stream), pageable source
    Event tier_ev;               // the bucket tiers' sizes have landed in pin_tier
    Event pin_up_ev;             // the last upload out of pin_up (on whichever stream queued it)
    Event cmp_ev;                // "this context's result is complete", on its stream, for another context's comparison
    Event xstage_ev;             // the staging stream's work so far (the count waits for it)
    Event emit_ev;               // map stream: a piece's send records are written
    std::vector<Event> fq_evs;   // begin / end of every normalise launch of the job (fk_debug_fastq_ms)
    std::vector<Event> seg_evs;  // fk_ingest, pinned source: one "segment landed" event per segment
    std::vector<Event> map_evs;  // ... and one "segment mapped" event (one rank's staged pieces)
    std::vector<Event> xev;      // comm stream: begin / end of every piece's transfer
    // pinned host memory
    PinBuf pinned[2];                     // staging for pageable sources
    PinBuf pin_up, pin_down;              // staging: chunk tables up, per-bin counts down
    bool pin_up_busy = false;             // pin_up's last upload was queued and not yet waited for
    PinBuf pin_tier;                      // the bucket tiers' sizes, read while the wave tier runs
    PinBuf file_pin[2];                   // fk_ingest_file_range: the split read in pinned windows
    PinBuf fq_pin;                        // fq_info read back with the map's counters
    PinBuf fold_pin;                      // the folded pieces' entries (one word per piece)
    PinBuf hold_flag;                     // fk_debug_comm_hold: host-mapped release flag
    // the input: host bytes are streamed to fasta_own (appended until the next fk_map); d_fasta is it, or
    // a borrowed device input (fk_ingest_device)
    DevBuf fasta_own;
    const uint8_t *d_fasta = nullptr;
    uint64_t n_fasta = 0;
    bool ingest_fresh = true;     // the next fk_ingest starts a new input
    DevBuf fq_ws, fq_info;        // FASTQ (fk_fastq.inc): launch workspace; the job's records, masked bases, ~(first bad record), overflow
    // parse + encode
    DevBuf tile_last_nl, tile_off, npos_dev, codes, valid;
    // signature
    DevBuf records, counters, sig_status, sig_kmers;
    DevBuf tcnt;                  // fused map: records per tile (tiled record layout)
    DevBuf rec_hdr;               // fused map: every record's header word, in the record's tile slot
    DevBuf rec_pos;               // fused map: every record's first position in its tile's code stream (u16)
    DevBuf rec_code;              // fused map: per tile, the tile's 2-bit code stream (map_fused_cslot() words)
    DevBuf tstat;                 // fused map: per tile (k-mers, positions)
    DevBuf map_vslots;            // split map: the parse kernel's valid streams for the passes (MAP_VSLOT_TILES tiles)
    // reduce
    PartBufs dest, part, binhist;  // record partition by destination rank (fk_map) / by local bin (fk_reduce)
    DevBuf precs, chunks, bin_chunk_begin;
    std::vector<uint32_t> h_bcb;  // bin_chunk_begin on the host (the last uploaded chunk table)
    DevBuf hpieces, hpiece_first, hpiece_tot;  // k_expand_hist_piece: bins split into pieces of chunks
    DevBuf chunk_nk, chunk_base, lp, cell_total, cell_base, flags, flag_scan, buckets, keys, out_keys, out_counts;
    DevBuf scratch;
    DevBuf bucket_unique, dense_off, dense_keys, dense_counts, bin_off, misc, tier_list, mid, sc_total;
    DevBuf sp_base, sp_keys, sp_subs, sp_par, sp_fb;  // heavy buckets split into sub-buckets
    DevBuf mid_fb;  // mid-tier buckets left to the 1024-key kernel by the ranges kernel
    // staged pieces (one rank, or the received segments with a communicator; sorted count, k <= 63):
    // each piece of the input is partitioned and expanded into its own key array while later pieces
    // land; the job's buckets are counted once over every piece's keys (no per-piece count, no merge)
    DevBuf st_keys[STAGE_MAXP], st_cb[STAGE_MAXP], st_total, piece_starts;
    DevBuf fold_cnt, fold_cb, fold_io;           // the fold: entries per cell, their scan, the sample's (keys, entries)
    DevBuf xsend, xrecv;                         // the exchange: send ring (pieces in flight), received records
    ViewBufs vw;
    std::vector<uint64_t> seg_tiles;  // scratch of one fk_ingest call: the tiles mapped once each segment's map is done

    // ---- 3. settings of the next job: they survive a job's begin
    int32_t in_format = FK_FORMAT_FASTA, fq_min_q = 0, fq_q_off = 33;  // fk_set_input_format
    uint64_t reserve_bytes = 0;   // fk_ingest_reserve's size for the next job
    // size-aware placement (fk_set_bin_owners): bin -> rank, bin -> local index, local index -> bin
    bool custom_owners = false;
    std::vector<int32_t> h_owner, h_lbin_bin;
    std::vector<uint32_t> h_bin_lbin;
    DevBuf d_owner, d_local;  // REC_BIN_MASK + 1 entries each (~0u: no part), device copies of the above
    // grouped emit (fk_set_grouped_emit): send buffer grouped by (destination, local bin)
    bool grouped = false;
    uint32_t grp_nlb = 0;                    // parts per destination = ceil(Bc / n_ranks)
    DevBuf grp_table;                        // bin -> dest * grp_nlb + bin / n_ranks

    // ---- 4. the job in flight, from its first ingest (begin_job, the one place that starts it) to its
    // count.  Pieces is the part that ends with the count as well, so that a second fk_finish counts
    // the whole input.
    struct XSeg {                                // received records of one (piece, sender)
        uint64_t off;                            // first record in xrecv
        int32_t sender;
        uint64_t step;                           // the exchange step that delivered it
        std::vector<uint64_t> rec, kmer;         // per local bin
    };
    struct Xch {                     // the exchange inside the context (fk_comm_init / fk_comm_init_local): the input
                                     // is emitted in pieces grouped by (destination, local bin), each exchanged while
                                     // the next one is copied in; fk_finish sends the last, then counts every segment
        bool open = false;           // a job's exchange has started (pieces sent)
        bool sent_final = false;     // this rank has sent its last piece
        bool all_final = false;      // every rank has sent its last piece
        bool stop_pieces = false;    // the fused map fell back: the rest goes in fk_finish, earlier pieces retracted
        uint64_t tiles_sent = 0;     // tiled records [0, tiles_sent) emitted in pieces
        uint64_t send_used = 0, recv_used = 0;  // records
        uint64_t pieces = 0, bytes_sent = 0, bytes_received = 0, expect_bytes = 0;
        std::vector<XSeg> segs;
    };
    struct Pieces {
        bool pieces_void = false;     // a fallback or a retract: the job is counted whole at the end
        uint64_t tiles_counted = 0;   // one rank: tiled records [0, tiles_counted) staged
        size_t segs_counted = 0;      // with a communicator: received segments [0, segs_counted) staged
        uint32_t st_np = 0;           // pieces expanded
        uint32_t st_cut = 0;          // one rank: st_cuts passed
        uint64_t st_kmers = 0;        // k-mers expanded so far
        bool st_weighted = false;     // the pieces hold weighted keys as given, no fold ran (fk_debug_count_pieces)
        // the fold of a landed piece (one rank, 64-bit keys with 2k <= 60): its duplicate k-mers become
        // weighted keys while later pieces land (fold_piece)
        bool fold_decided = false, fold_on = false;  // the job's gate (mode 1: set by its first piece's sample)
        uint64_t fold_sample_ppm = 0;                // ... entries per million sampled keys (0: no sample taken)
        uint64_t fold_in = 0;                        // keys of the job's folded pieces
        std::vector<uint32_t> fold_pieces;           // ... the pieces (their entries: the last word of st_cb[p])
    };
    struct Job : Pieces {
        bool job_open = false;      // between the first ingest and fk_map / fk_finish
        bool dev_open = false;      // fk_ingest_device(..., last = 0): the borrowed input is unfinished
        uint64_t job_bytes = 0;     // one rank: the input's size when one fk_ingest call holds it all, or
                                    // announced by fk_ingest_reserve (0: unknown)
        // streamed map (fused path): fk_ingest maps every tile whose bytes (and halo) have landed
        bool pm_active = false;     // the input is being mapped while it is copied
        uint64_t pm_tiles = 0;      // tiles [0, pm_tiles) launched
        bool pm_last_seen = false;  // an fk_ingest with last = 1 launched the final tiles
        // FASTQ: the device input is normalised in place to text the FASTA parsers read, record-aligned
        // range after range, each byte once
        bool fq_job = false;        // the input is FASTQ
        uint64_t fq_done = 0;       // the frontier: bytes [0, fq_done) are normalised (and may be mapped)
        std::vector<uint8_t> fq_tail;  // host copy of the caller's bytes [fq_done, n_fasta) (a record straddling two calls)
        bool fq_launched = false;   // a normalise launch has been queued
        size_t fq_nev = 0;          // fq_evs used
        SortedPlan st_plan;         // the staged pieces' cells (fixed by the first piece)
        Xch xch;
    } job;

    // ---- 5. the last map and the last result, until the next job clears them (new_result, reset_results)
    bool mapped = false;
    bool rec_tiled = false;       // records: the fused map's tiles (else dense, nrec)
    uint64_t rec_tiles = 0;       // tiles of the tiled layout
    uint64_t nrec = 0, nkmers = 0;
    bool last_map_fused = false;  // the last fk_map used the fused kernel (stats, tests)
    std::vector<uint64_t> send_counts;       // destination partition (n_ranks > 1)
    std::vector<uint64_t> grp_rec, grp_kmer; // grouped emit: per part, after fk_map
    const uint64_t *rsrc = nullptr;          // records the count stage reads (precs, or d_recv when grouped)
    bool have_result = false;
    uint64_t distinct = 0;
    bool distinct_pending = false;        // the sorted count's distinct total arrives with the bin offsets
    std::vector<uint64_t> h_bin_off;  // [nlb + 1]
    fk_stats stats{};
    double ms_h2d = 0.0;  // last fk_ingest: first copy issued -> last copy done
    // The sorted count's result is bucket-major ("gapped"): bucket q's distinct keys ascending at its
    // first slot buckets[q].begin of res_keys / out_counts, dense_off[q] = their exclusive offset in the
    // bin-ordered result, bin_off / h_bin_off per bin.  Readers gather a bin's buckets (fk_get_bin) or
    // the whole result (fk_write_bins).
    bool gapped = false, dense_ready = false;
    const uint64_t *res_keys = nullptr;   // okb of the last sorted count (out_keys, or mid)
    const uint64_t *res_fs = nullptr;     // flag_scan of its bucket cut
    uint64_t res_nbuckets = 0;
    int res_F = 0;
    // the last job's figures, read by debug calls
    bool fq_have_info = false;  // fk_fastq_info has figures (a FASTQ job was mapped)
    uint64_t fq_out[3] = {0, 0, UINT64_MAX};
    uint64_t fold_last[4] = {0, 0, 0, 0};        // fk_debug_fold_stats
    // the last tiered count's census, from the figures its driver read anyway: [0] mid-tier buckets handed
    // on, [1] / [2] split fallbacks of at most / above cap keys, [3] buckets on the streaming path,
    // [4] the mid tier's first kernel (0 none, 1 key ranges, 2 whole on the 512-key table)
    uint64_t tier_last[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t last_np = 0;                        // the last staged count's pieces and cells (fk_debug_staged_piece)
    uint64_t last_cells = 0;
    double store_ms[8] = {};              // the last fk_save / fk_load / fk_import* (fk_debug_store_ms)
};

// fk_api.cpp, shared with fk_store.cpp: the cells of a count whose largest bin holds max_bin_kmers keys, and
// "the context holds no result"
SortedPlan sorted_plan(const fk_ctx *c, uint64_t max_bin_kmers, int force_F = 0);
void reset_results(fk_ctx *c);

// How bins map to ranks and to a rank's local bins (default placement, or fk_set_bin_owners).
inline const uint32_t *owner_table(const fk_ctx *c) { return c->custom_owners ? c->d_owner.as<uint32_t>() : nullptr; }
inline const uint32_t *local_table(const fk_ctx *c) { return c->custom_owners ? c->d_local.as<uint32_t>() : nullptr; }
inline int32_t global_bin(const fk_ctx *c, uint32_t lb) {
    return c->custom_owners ? c->h_lbin_bin[lb] : (int32_t)(c->cfg.rank + lb * c->G);
}
inline bool owns(const fk_ctx *c, int32_t b) {
    if (b < 0 || b >= c->Bc) return false;
    return c->custom_owners ? c->h_owner[b] == c->cfg.rank : (uint32_t)b % c->G == (uint32_t)c->cfg.rank;
}
inline uint32_t local_bin(const fk_ctx *c, int32_t b) { return c->custom_owners ? c->h_bin_lbin[b] : (uint32_t)b / c->G; }
inline int32_t bin_owner(const fk_ctx *c, int32_t b) {
    return c->custom_owners ? c->h_owner[b] : (int32_t)((uint32_t)b % c->G);
}
