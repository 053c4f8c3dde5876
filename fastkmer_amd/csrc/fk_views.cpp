// fk_views.cpp -- the C-ABI calls that only read a finished result (include/fastkmer.h): bins, lookups,
// bin files, the spectrum, filtered bins, the two-sample comparison, per-read profiles.  The result is the
// context's (fk_ctx.h), left bucket-major by the count in fk_api.cpp.  The calls stage through the
// context's grow-only ViewBufs; what spans the whole result is a call's own DevBuf.
#include <errno.h>
#include <stdio.h>
#include <string.h>
#include <sys/stat.h>

#include <cstdlib>
#include <thread>

#include "fk_ctx.h"

// ---------------------------------------------------------------------------
// results
// ---------------------------------------------------------------------------

// out[b] = bin b's size by the offsets off[0 .. nlb] of this rank's local bins, 0 for another rank's bin
static void owned_bin_sizes(const fk_ctx *c, const std::vector<uint64_t> &off, uint64_t *out) {
    for (int32_t b = 0; b < c->Bc; ++b) out[b] = owns(c, b) ? off[local_bin(c, b) + 1] - off[local_bin(c, b)] : 0;
}

FK_EXPORT int fk_bin_sizes(fk_ctx *c, uint64_t *out) {
    if (!c || !out) return set_err(FK_E_INVALID, "null argument");
    if (!c->have_result) return set_err(FK_E_STATE, "no result: call fk_finish or fk_reduce first");
    owned_bin_sizes(c, c->h_bin_off, out);
    return FK_OK;
}

// A bucket-major result made dense (fk_write_bins): the buckets' outputs compacted in bin order.
static int materialize_dense(fk_ctx *c) {
    if (!c->gapped || c->dense_ready) return FK_OK;
    hipStream_t s = c->stream;
    FK_TRY(ensure(c->dense_keys, c->distinct * 8 * c->KW));
    FK_TRY(ensure(c->dense_counts, c->distinct * 4));
    HIP_TRY(launch_bucket_compact(c->KW, c->res_keys, c->out_counts.as<uint32_t>(), c->buckets.as<Bucket>(),
                                  c->res_nbuckets, c->dense_off.as<uint64_t>(), c->dense_keys.as<uint64_t>(),
                                  c->dense_counts.as<uint32_t>(), s));
    HIP_TRY(hipStreamSynchronize(s));
    c->dense_ready = true;
    return FK_OK;
}

// A local bin's buckets [q[0], q[1]) of a bucket-major result: the bin's first cell starts a bucket,
// so q0 = flag_scan[lb << F]; the last local bin ends with the result's buckets.
static int bin_buckets(fk_ctx *c, uint32_t lb, uint64_t q[2]) {
    hipStream_t s = c->stream;
    q[0] = 0, q[1] = c->res_nbuckets;
    const uint64_t *fs = c->res_fs;
    HIP_TRY(hipMemcpyAsync(&q[0], fs + ((uint64_t)lb << c->res_F), 8, hipMemcpyDeviceToHost, s));
    if (lb + 1 < c->nlb) HIP_TRY(hipMemcpyAsync(&q[1], fs + ((uint64_t)(lb + 1) << c->res_F), 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return FK_OK;
}

// One local bin of a bucket-major result into dst (device): its buckets compacted at dense_off[q] - dense_off[q0].
static int gather_bin(fk_ctx *c, uint32_t lb, uint64_t *dkeys, uint32_t *dcounts) {
    hipStream_t s = c->stream;
    uint64_t q[2];
    FK_TRY(bin_buckets(c, lb, q));
    const uint64_t d0 = c->h_bin_off[lb];
    if (q[1] > q[0])
        HIP_TRY(launch_bucket_compact(c->KW, c->res_keys, c->out_counts.as<uint32_t>(), c->buckets.as<Bucket>() + q[0],
                                      q[1] - q[0], c->dense_off.as<uint64_t>() + q[0], dkeys - d0 * c->KW, dcounts - d0, s));
    return FK_OK;
}

FK_EXPORT int fk_get_bin(fk_ctx *c, int32_t bin, uint64_t *keys, uint32_t *counts, size_t cap, size_t *n) {
    if (!c || !n) return set_err(FK_E_INVALID, "null argument");
    DeviceGuard dg_(c->device);
    if (!c->have_result) return set_err(FK_E_STATE, "no result: call fk_finish or fk_reduce first");
    if (bin < 0 || bin >= c->Bc) return set_err(FK_E_RANGE, "bin %d out of [0, %d)", bin, c->Bc);
    if (!owns(c, bin)) {
        *n = 0;
        return FK_OK;
    }
    const uint32_t lb = local_bin(c, bin);
    const uint64_t b0 = c->h_bin_off[lb], cnt = c->h_bin_off[lb + 1] - b0;
    *n = (size_t)cnt;
    if (cnt == 0) return FK_OK;
    if (cap < cnt) return set_err(FK_E_RANGE, "bin %d has %llu k-mers, buffer holds %zu", bin, (unsigned long long)cnt, cap);
    if (c->gapped && !c->dense_ready) {
        FK_TRY(ensure(c->vw.gather_keys, cnt * 8 * c->KW));
        FK_TRY(ensure(c->vw.gather_counts, cnt * 4));
        FK_TRY(gather_bin(c, lb, c->vw.gather_keys.as<uint64_t>(), c->vw.gather_counts.as<uint32_t>()));
        if (keys)
            HIP_TRY(hipMemcpyAsync(keys, c->vw.gather_keys.p, cnt * 8 * c->KW, hipMemcpyDeviceToHost, c->stream));
        if (counts) HIP_TRY(hipMemcpyAsync(counts, c->vw.gather_counts.p, cnt * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        return FK_OK;
    }
    if (keys)
        HIP_TRY(hipMemcpy(keys, c->dense_keys.as<uint64_t>() + b0 * c->KW, cnt * 8 * c->KW, hipMemcpyDeviceToHost));
    if (counts) HIP_TRY(hipMemcpy(counts, c->dense_counts.as<uint32_t>() + b0, cnt * 4, hipMemcpyDeviceToHost));
    return FK_OK;
}

// ---------------------------------------------------------------------------
// lookups in the counted result (fk_query.inc)
// ---------------------------------------------------------------------------

// keys (or windows) per staged chunk of fk_query / fk_query_sequence: FASTKMER_QUERY_CHUNK, default 16 Mi
static uint64_t query_chunk() {
    const char *v = getenv("FASTKMER_QUERY_CHUNK");
    const uint64_t n = v && v[0] ? strtoull(v, nullptr, 10) : 0;
    return n ? n : 16ull << 20;
}

// the sorted count's bucket-major arrays as the lookup kernel reads them
static int query_tables(fk_ctx *c, QueryTables &t) {
    if (c->cfg.use_ht) return set_err(FK_E_INVALID, "%s", MSG_NEED_SORTED);
    if (!c->have_result || !c->gapped) return set_err(FK_E_STATE, "no result: call fk_finish or fk_reduce first");
    t.flag_scan = c->res_fs;
    t.buckets = c->buckets.as<Bucket>();
    t.dense_off = c->dense_off.as<uint64_t>();
    t.keys = c->res_keys;
    t.counts = c->out_counts.as<uint32_t>();
    t.owner = owner_table(c);
    t.local = local_table(c);
    t.nbuckets = c->res_nbuckets;
    t.fm = c->fm;
    t.G = c->G;
    t.rank = (uint32_t)c->cfg.rank;
    t.nlb = c->nlb;
    t.k = c->cfg.k;
    t.m = c->cfg.m;
    t.F = c->res_F;
    return FK_OK;
}

FK_EXPORT int fk_kmer_bin(const fk_config *cfg, const uint64_t *key, int32_t *bin) {
    if (!cfg || !key || !bin) return set_err(FK_E_INVALID, "null argument");
    FK_TRY(fk_config_validate(cfg));
    const int k = cfg->k;
    const KmerKey f = k > 32 ? KmerKey{key[0], key[1]} : KmerKey{0, key[0]};
    if (!key_is_kmer(f, k)) return set_err(FK_E_INVALID, "the key has a bit set above bit 2k - 1 = %d", 2 * k - 1);
    const uint32_t sig = k > 32 ? kmer_signature<true>(f, revcomp_key<true>(f, k), k, cfg->m)
                                : kmer_signature<false>(f, revcomp_key<false>(f, k), k, cfg->m);
    *bin = (int32_t)bin_of_signature(sig, make_fastmod((uint32_t)clamp_bins(cfg->m, cfg->B)));
    return FK_OK;
}

FK_EXPORT int fk_query_device(fk_ctx *c, const void *d_keys, size_t n, void *d_counts, void *d_bins) {
    if (!c) return set_err(FK_E_INVALID, "null ctx");
    DeviceGuard dg_(c->device);
    QueryTables t;
    FK_TRY(query_tables(c, t));
    if (n == 0) return FK_OK;
    if (!d_keys || !d_counts) return set_err(FK_E_INVALID, "null argument");
    HIP_TRY(launch_query(c->KW, t, static_cast<const uint64_t *>(d_keys), n, static_cast<uint32_t *>(d_counts),
                         static_cast<int32_t *>(d_bins), c->stream));
    return FK_OK;
}

FK_EXPORT int fk_query(fk_ctx *c, const uint64_t *keys, size_t n, uint32_t *counts, int32_t *bins) {
    if (!c) return set_err(FK_E_INVALID, "null ctx");
    DeviceGuard dg_(c->device);
    QueryTables t;
    FK_TRY(query_tables(c, t));
    if (n == 0) return FK_OK;
    if (!keys || !counts) return set_err(FK_E_INVALID, "null argument");
    hipStream_t s = c->stream;
    const size_t chunk = (size_t)std::min<uint64_t>(query_chunk(), n), kb = (size_t)c->KW * 8;
    FK_TRY(ensure(c->vw.q_in, chunk * kb));
    FK_TRY(ensure(c->vw.q_counts, chunk * 4));
    if (bins) FK_TRY(ensure(c->vw.q_bins, chunk * 4));
    for (size_t at = 0; at < n; at += chunk) {
        const size_t nc = std::min(chunk, n - at);
        HIP_TRY(hipMemcpyAsync(c->vw.q_in.p, keys + at * c->KW, nc * kb, hipMemcpyHostToDevice, s));
        HIP_TRY(launch_query(c->KW, t, c->vw.q_in.as<uint64_t>(), nc, c->vw.q_counts.as<uint32_t>(),
                             bins ? c->vw.q_bins.as<int32_t>() : nullptr, s));
        HIP_TRY(hipMemcpyAsync(counts + at, c->vw.q_counts.p, nc * 4, hipMemcpyDeviceToHost, s));
        if (bins) HIP_TRY(hipMemcpyAsync(bins + at, c->vw.q_bins.p, nc * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));  // the staging buffers are free for the next chunk
    }
    return FK_OK;
}

FK_EXPORT int fk_query_sequence(fk_ctx *c, const uint8_t *seq, size_t len, uint32_t *counts, size_t cap, size_t *n) {
    if (!c || !n) return set_err(FK_E_INVALID, "null argument");
    DeviceGuard dg_(c->device);
    QueryTables t;
    FK_TRY(query_tables(c, t));
    const size_t k = (size_t)c->cfg.k, nwin = len >= k ? len - k + 1 : 0;
    *n = nwin;
    if (!counts || nwin == 0) return FK_OK;
    if (cap < nwin) return set_err(FK_E_RANGE, "the sequence has %zu windows, buffer holds %zu", nwin, cap);
    if (!seq) return set_err(FK_E_INVALID, "null argument");
    hipStream_t s = c->stream;
    // windows [at, at + nc) read the bases [at, at + nc + k - 1): packed on the device (k_query_seq)
    const size_t chunk = (size_t)std::min<uint64_t>(query_chunk(), nwin);
    FK_TRY(ensure(c->vw.q_in, chunk + k - 1));
    FK_TRY(ensure(c->vw.q_counts, chunk * 4));
    for (size_t at = 0; at < nwin; at += chunk) {
        const size_t nc = std::min(chunk, nwin - at);
        HIP_TRY(hipMemcpyAsync(c->vw.q_in.p, seq + at, nc + k - 1, hipMemcpyHostToDevice, s));
        HIP_TRY(launch_query_seq(c->KW, t, c->vw.q_in.as<uint8_t>(), nc, c->vw.q_counts.as<uint32_t>(), s));
        HIP_TRY(hipMemcpyAsync(counts + at, c->vw.q_counts.p, nc * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    return FK_OK;
}

int fk::mkdir_p(const std::string &path) {
    std::string cur;
    for (size_t i = 0; i < path.size(); ++i) {
        cur.push_back(path[i]);
        if ((path[i] == '/' && i > 0) || i + 1 == path.size()) {
            if (mkdir(cur.c_str(), 0755) != 0 && errno != EEXIST) return -1;
        }
    }
    return 0;
}

// Bin files (writers SBKC:550-606 / 715-734) of D dense lines (device keys / counts in bin order,
// bin_off / h_bin_off their nlb + 1 offsets per local bin on the device / host): the text is
// formatted on the device (fk_format.inc), copied to the host once and written one file per bin.
static int write_bin_text(fk_ctx *c, const char *out_dir, const uint64_t *keys, const uint32_t *counts, uint64_t D,
                          const uint64_t *bin_off, const std::vector<uint64_t> &h_bin_off) {
    hipStream_t s = c->stream;
    const uint32_t nlb = c->nlb;
    const int eof = c->cfg.use_ht == 0;
    if (D == 0) return FK_OK;  // no k-mers: no bin files
    DevBuf len, off, bbytes, text;
    FK_TRY(ensure(len, D * 4));
    FK_TRY(ensure(off, (D + 1) * 8));
    FK_TRY(ensure(bbytes, ((uint64_t)nlb + 1) * 8));
    HIP_TRY(launch_format_lens(counts, D, c->cfg.k, bin_off, nlb, eof, len.as<uint32_t>(), s));
    HIP_TRY(scan_excl_sum_u32_to_u64(len.as<uint32_t>(), off.as<uint64_t>(), D, off.as<uint64_t>() + D, c->ws, s));
    HIP_TRY(launch_gather_u64(off.as<uint64_t>(), bin_off, (uint64_t)nlb + 1, bbytes.as<uint64_t>(), s));
    std::vector<uint64_t> bb(nlb + 1, 0);
    HIP_TRY(hipMemcpyAsync(bb.data(), bbytes.p, ((uint64_t)nlb + 1) * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const uint64_t T = bb[nlb];
    FK_TRY(ensure(text, T + 16));
    HIP_TRY(launch_format_lines(c->KW, keys, counts, D, c->cfg.k, off.as<uint64_t>(), text.as<uint8_t>(), s));
    PinBuf pin;
    if (T) {
        HIP_TRY(pin.alloc(T, hipHostMallocDefault));
        const hipError_t e = hipMemcpyAsync(pin.p, text.p, T, hipMemcpyDeviceToHost, s);
        const hipError_t e2 = e == hipSuccess ? hipStreamSynchronize(s) : e;
        if (e2 != hipSuccess) return set_err(FK_E_DEVICE, "copying the bin text to the host: %s", hipGetErrorString(e2));
    }
    const uint8_t *host = pin.as<uint8_t>();
    const std::string dir(out_dir);
    const unsigned nth = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    std::vector<int> errs(nth, 0);
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nth; ++t) {
        th.emplace_back([&, t]() {
            for (uint32_t lb = t; lb < nlb; lb += nth) {
                if (h_bin_off[lb + 1] == h_bin_off[lb]) continue;  // empty bins have no file
                const std::string path = dir + "/bin" + std::to_string(global_bin(c, lb));
                FILE *f = fopen(path.c_str(), "wb");
                const size_t nb = (size_t)(bb[lb + 1] - bb[lb]);
                if (!f || fwrite(host + bb[lb], 1, nb, f) != nb) errs[t] = 1;
                if (f && fclose(f) != 0) errs[t] = 1;
            }
        });
    }
    for (auto &x : th) x.join();
    for (int e : errs)
        if (e) return set_err(FK_E_IO, "writing bin files under %s failed", out_dir);
    return FK_OK;
}

FK_EXPORT int fk_write_bins(fk_ctx *c, const char *out_dir) {
    if (!c || !out_dir) return set_err(FK_E_INVALID, "null argument");
    DeviceGuard dg_(c->device);
    if (!c->have_result) return set_err(FK_E_STATE, "no result: call fk_finish or fk_reduce first");
    if (mkdir_p(out_dir) != 0) return set_err(FK_E_IO, "cannot create %s: %s", out_dir, strerror(errno));
    if (c->distinct == 0) return FK_OK;  // no k-mers: no bin files
    FK_TRY(materialize_dense(c));
    return write_bin_text(c, out_dir, c->dense_keys.as<uint64_t>(), c->dense_counts.as<uint32_t>(), c->distinct,
                          c->bin_off.as<uint64_t>(), c->h_bin_off);
}

// ---------------------------------------------------------------------------
// abundance spectrum of the counted result (fk_spectrum.inc); either count mode
// ---------------------------------------------------------------------------

static int result_ready(const fk_ctx *c) {
    if (!c->have_result) return set_err(FK_E_STATE, "no result: call fk_finish or fk_reduce first");
    if (c->distinct && !c->gapped) return set_err(FK_E_STATE, "the result is not bucket-major");
    return FK_OK;
}

static int check_count_range(uint32_t lo, uint32_t hi) {
    if (lo == 0) return set_err(FK_E_INVALID, "min_count must be >= 1 (no k-mer of the result has count 0)");
    if (lo > hi) return set_err(FK_E_INVALID, "min_count %u > max_count %u", lo, hi);
    return FK_OK;
}

static int spectrum_launch(fk_ctx *c, uint64_t *d_hist, size_t n, uint64_t *d_tail) {
    // an empty job has no buckets: the launcher only clears the outputs
    HIP_TRY(launch_spectrum(c->out_counts.as<uint32_t>(), c->buckets.as<Bucket>(), c->dense_off.as<uint64_t>(),
                            c->distinct ? c->res_nbuckets : 0, c->spectrum_wide ? ~0ull : c->distinct, d_hist, n, d_tail,
                            c->stream));
    return FK_OK;
}

FK_EXPORT int fk_spectrum_device(fk_ctx *c, void *d_hist, size_t n, void *d_tail_kmers) {
    if (!c) return set_err(FK_E_INVALID, "null ctx");
    DeviceGuard dg_(c->device);
    FK_TRY(result_ready(c));
    if (n < 2) return set_err(FK_E_INVALID, "a spectrum has n >= 2 entries");
    if (!d_hist) return set_err(FK_E_INVALID, "null argument");
    return spectrum_launch(c, static_cast<uint64_t *>(d_hist), n, static_cast<uint64_t *>(d_tail_kmers));
}

FK_EXPORT int fk_spectrum(fk_ctx *c, uint64_t *hist, size_t n, uint64_t *tail_kmers) {
    if (!c) return set_err(FK_E_INVALID, "null ctx");
    DeviceGuard dg_(c->device);
    FK_TRY(result_ready(c));
    if (n < 2) return set_err(FK_E_INVALID, "a spectrum has n >= 2 entries");
    if (!hist) return set_err(FK_E_INVALID, "null argument");
    FK_TRY(ensure(c->vw.sp_hist, ((uint64_t)n + 1) * 8));
    uint64_t *d = c->vw.sp_hist.as<uint64_t>();
    FK_TRY(spectrum_launch(c, d, n, d + n));
    HIP_TRY(hipMemcpyAsync(hist, d, (uint64_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    if (tail_kmers) HIP_TRY(hipMemcpyAsync(tail_kmers, d + n, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return FK_OK;
}

// ---------------------------------------------------------------------------
// two-sample comparison (fk_compare.inc): c's result walked, o's looked up in
// ---------------------------------------------------------------------------

// both contexts count the same k-mers into the same bins of the same rank, and hold a result
static int compare_pair(const fk_ctx *c, const fk_ctx *o) {
    if (c->cfg.use_ht || o->cfg.use_ht)
        return set_err(FK_E_INVALID, "a comparison needs the sorted count (use_ht = 0) on both contexts: a use_ht = 1 "
                                     "result is in table order");
    if (c->cfg.k != o->cfg.k) return set_err(FK_E_INVALID, "the contexts differ in k: %d and %d", c->cfg.k, o->cfg.k);
    if (c->cfg.m != o->cfg.m) return set_err(FK_E_INVALID, "the contexts differ in m: %d and %d", c->cfg.m, o->cfg.m);
    if (c->Bc != o->Bc) return set_err(FK_E_INVALID, "the contexts differ in their bin count: %d and %d", c->Bc, o->Bc);
    if (c->G != o->G) return set_err(FK_E_INVALID, "the contexts differ in n_ranks: %u and %u", c->G, o->G);
    if (c->cfg.rank != o->cfg.rank)
        return set_err(FK_E_INVALID, "the contexts differ in rank: %d and %d", c->cfg.rank, o->cfg.rank);
    if (c->device != o->device)
        return set_err(FK_E_INVALID, "the contexts are on different devices: %d and %d", c->device, o->device);
    if (c->custom_owners || o->custom_owners)
        for (int32_t b = 0; b < c->Bc; ++b)
            if (bin_owner(c, b) != bin_owner(o, b))
                return set_err(FK_E_INVALID, "the contexts differ in their bin owners: bin %d belongs to rank %d and to rank %d",
                               b, bin_owner(c, b), bin_owner(o, b));
    if (!c->have_result || !o->have_result)
        return set_err(FK_E_STATE, "no result on %s: call fk_finish or fk_reduce first",
                       !c->have_result ? "the walked context" : "the other context");
    return FK_OK;
}

// a context's result as the comparison kernels read it; an empty job: no bucket to walk, every lookup 0
static int compare_tables(fk_ctx *c, QueryTables &t) {
    if (c->distinct) return query_tables(c, t);
    t = QueryTables{};
    t.fm = c->fm;
    t.G = 1;
    t.k = c->cfg.k;
    t.m = c->cfg.m;
    return FK_OK;
}

// c's stream waits for everything queued on o's: o's result arrays are complete when c's kernels read them
static int compare_order(fk_ctx *c, fk_ctx *o) {
    if (o == c || o->stream == c->stream) return FK_OK;
    HIP_TRY(hipEventRecord(o->cmp_ev, o->stream));
    HIP_TRY(hipStreamWaitEvent(c->stream, o->cmp_ev, 0));
    return FK_OK;
}

static int check_matrix_shape(size_t rows, size_t cols) {
    if (rows < 2 || cols < 2 || rows > 65536 || cols > 65536 || (uint64_t)rows * cols > (1ull << 24))
        return set_err(FK_E_INVALID, "a comparison matrix has 2 <= rows, cols <= 65536 and rows * cols <= 2^24 (got %zu x %zu)",
                       rows, cols);
    return FK_OK;
}

static uint64_t walk_width(const fk_ctx *c) { return c->spectrum_wide ? ~0ull : c->distinct; }

static int compare_launch(fk_ctx *c, fk_ctx *o, uint64_t *d_matrix, size_t rows, size_t cols) {
    QueryTables ta, tb;
    FK_TRY(compare_tables(c, ta));
    FK_TRY(compare_tables(o, tb));
    FK_TRY(compare_order(c, o));
    HIP_TRY(launch_compare(c->KW, ta, tb, walk_width(c), d_matrix, (uint32_t)rows, (uint32_t)cols, false, c->stream));
    // the k-mers only o holds (every k-mer of c's own result is found in it: nothing to add)
    if (o != c)
        HIP_TRY(launch_compare(c->KW, tb, ta, walk_width(o), d_matrix, (uint32_t)rows, (uint32_t)cols, true, c->stream));
    return FK_OK;
}

FK_EXPORT int fk_compare_device(fk_ctx *c, fk_ctx *o, void *d_matrix, size_t rows, size_t cols) {
    if (!c || !o) return set_err(FK_E_INVALID, "null ctx");
    DeviceGuard dg_(c->device);
    FK_TRY(check_matrix_shape(rows, cols));
    FK_TRY(compare_pair(c, o));
    if (!d_matrix) return set_err(FK_E_INVALID, "null argument");
    return compare_launch(c, o, static_cast<uint64_t *>(d_matrix), rows, cols);
}

FK_EXPORT int fk_compare(fk_ctx *c, fk_ctx *o, uint64_t *matrix, size_t rows, size_t cols) {
    if (!c || !o) return set_err(FK_E_INVALID, "null ctx");
    DeviceGuard dg_(c->device);
    FK_TRY(check_matrix_shape(rows, cols));
    FK_TRY(compare_pair(c, o));
    if (!matrix) return set_err(FK_E_INVALID, "null argument");
    const uint64_t bytes = (uint64_t)rows * cols * 8;
    FK_TRY(ensure(c->vw.cmp_mat, bytes));
    FK_TRY(compare_launch(c, o, c->vw.cmp_mat.as<uint64_t>(), rows, cols));
    HIP_TRY(hipMemcpyAsync(matrix, c->vw.cmp_mat.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return FK_OK;
}

static int check_join_range(uint32_t lo, uint32_t hi, uint32_t olo, uint32_t ohi) {
    FK_TRY(check_count_range(lo, hi));
    if (olo > ohi) return set_err(FK_E_INVALID, "other_min %u > other_max %u", olo, ohi);
    return FK_OK;
}

// ---------------------------------------------------------------------------
// filtered views: by count range (fk_spectrum.inc; either count mode), or joined with another result (fk_compare.inc)
// ---------------------------------------------------------------------------

// A filtered view keeps the k-mers with a count in [lo, hi] and, where o is given, one in [olo, ohi] in o's result.
struct Filter {
    uint32_t lo, hi;
    fk_ctx *o = nullptr;
    uint32_t olo = 0, ohi = 0;
    QueryTables walk, other;  // the buckets walked (buckets, dense_off, nbuckets; joined: all of it) / o's result
};

// Points f at c's whole result; joined, c's stream is ordered behind o's before any kernel reads o's arrays.
static int filter_bind(fk_ctx *c, Filter &f) {
    if (f.o) {
        FK_TRY(compare_tables(c, f.walk));
        FK_TRY(compare_tables(f.o, f.other));
        return compare_order(c, f.o);
    }
    f.walk.buckets = c->buckets.as<Bucket>();
    f.walk.dense_off = c->dense_off.as<uint64_t>();
    f.walk.nbuckets = c->res_nbuckets;
    return FK_OK;
}

// kept[i] = the k-mers of the i-th walked bucket that pass the filter
static int filter_count(fk_ctx *c, const Filter &f, uint64_t *kept) {
    const QueryTables &w = f.walk;
    if (f.o)
        HIP_TRY(launch_join_count(c->KW, w, f.other, f.lo, f.hi, f.olo, f.ohi, kept, c->stream));
    else
        HIP_TRY(launch_range_count(c->out_counts.as<uint32_t>(), w.buckets, w.dense_off, w.nbuckets, f.lo, f.hi, kept,
                                   c->stream));
    return FK_OK;
}

// ... written at koff, the exclusive scan of kept; other (joined only): their counts in o's result
static int filter_compact(fk_ctx *c, const Filter &f, const uint64_t *koff, uint64_t *keys, uint32_t *counts,
                          uint32_t *other) {
    const QueryTables &w = f.walk;
    if (f.o)
        HIP_TRY(launch_join_compact(c->KW, w, f.other, f.lo, f.hi, f.olo, f.ohi, koff, keys, counts, other, c->stream));
    else
        HIP_TRY(launch_range_compact(c->KW, c->res_keys, c->out_counts.as<uint32_t>(), w.buckets, w.dense_off, koff,
                                     w.nbuckets, f.lo, f.hi, keys, counts, c->stream));
    return FK_OK;
}

// The whole result filtered: kept k-mers per bucket -> their scan (off) -> offsets per local bin (d_off
// on the device, h_off their copy on the host).  kept / off / d_off: the caller's temporaries.  Binds f.
static int filtered_offsets(fk_ctx *c, Filter &f, DevBuf &kept, DevBuf &off, DevBuf &d_off, std::vector<uint64_t> &h_off) {
    FK_TRY(filter_bind(c, f));
    hipStream_t s = c->stream;
    const uint64_t nb = c->res_nbuckets;
    const uint32_t nlb = c->nlb;
    FK_TRY(ensure(kept, nb * 8));
    FK_TRY(ensure(off, (nb + 1) * 8));
    FK_TRY(ensure(d_off, ((uint64_t)nlb + 1) * 8));
    FK_TRY(filter_count(c, f, kept.as<uint64_t>()));
    HIP_TRY(scan_excl_sum_u64(kept.as<uint64_t>(), off.as<uint64_t>(), nb, off.as<uint64_t>() + nb, c->ws, s));
    HIP_TRY(launch_bin_offsets(c->res_fs, off.as<uint64_t>(), nlb, c->res_F, nb, d_off.as<uint64_t>(), s));
    h_off.assign((size_t)nlb + 1, 0);
    HIP_TRY(hipMemcpyAsync(h_off.data(), d_off.p, ((uint64_t)nlb + 1) * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return FK_OK;
}

// Every bin's filtered size into out[0 .. Bc).
static int filtered_bin_sizes(fk_ctx *c, Filter f, uint64_t *out) {
    for (int32_t b = 0; b < c->Bc; ++b) out[b] = 0;
    if (c->distinct == 0) return FK_OK;
    DevBuf kept, off, d_off;
    std::vector<uint64_t> h_off;
    FK_TRY(filtered_offsets(c, f, kept, off, d_off, h_off));
    owned_bin_sizes(c, h_off, out);
    return FK_OK;
}

// One bin filtered: the two filter kernels over the bin's buckets only, through the context's rg_* and
// gather_* buffers.  *n is the filtered size whatever cap is; each output may be null.
static int filtered_bin(fk_ctx *c, Filter f, int32_t bin, uint64_t *keys, uint32_t *counts, uint32_t *other_counts,
                        size_t cap, size_t *n) {
    if (bin < 0 || bin >= c->Bc) return set_err(FK_E_RANGE, "bin %d out of [0, %d)", bin, c->Bc);
    *n = 0;
    if (!owns(c, bin) || c->distinct == 0) return FK_OK;
    const uint32_t lb = local_bin(c, bin);
    if (c->h_bin_off[lb + 1] == c->h_bin_off[lb]) return FK_OK;
    FK_TRY(filter_bind(c, f));
    hipStream_t s = c->stream;
    uint64_t q[2];
    FK_TRY(bin_buckets(c, lb, q));
    if (q[1] <= q[0] || q[1] > c->res_nbuckets) return FK_OK;
    const uint64_t nq = q[1] - q[0];
    f.walk.buckets += q[0], f.walk.dense_off += q[0];  // the walk covers the bin's buckets only
    f.walk.nbuckets = nq;
    ViewBufs &v = c->vw;
    FK_TRY(ensure(v.rg_kept, nq * 8));
    FK_TRY(ensure(v.rg_off, (nq + 1) * 8));
    uint64_t *koff = v.rg_off.as<uint64_t>();
    FK_TRY(filter_count(c, f, v.rg_kept.as<uint64_t>()));
    HIP_TRY(scan_excl_sum_u64(v.rg_kept.as<uint64_t>(), koff, nq, koff + nq, c->ws, s));
    uint64_t cnt = 0;
    HIP_TRY(hipMemcpyAsync(&cnt, koff + nq, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *n = (size_t)cnt;
    if (cnt == 0) return FK_OK;
    if (cap < cnt)
        return f.o ? set_err(FK_E_RANGE, "bin %d has %llu k-mers with counts in [%u, %u] and [%u, %u] in the other result, buffer holds %zu",
                             bin, (unsigned long long)cnt, f.lo, f.hi, f.olo, f.ohi, cap)
                   : set_err(FK_E_RANGE, "bin %d has %llu k-mers with counts in [%u, %u], buffer holds %zu", bin,
                             (unsigned long long)cnt, f.lo, f.hi, cap);
    if (!keys && !counts && !other_counts) return FK_OK;
    FK_TRY(ensure(v.gather_keys, cnt * 8 * c->KW));
    FK_TRY(ensure(v.gather_counts, cnt * 4));
    if (f.o) FK_TRY(ensure(v.gather_other, cnt * 4));
    FK_TRY(filter_compact(c, f, koff, v.gather_keys.as<uint64_t>(), v.gather_counts.as<uint32_t>(),
                          f.o ? v.gather_other.as<uint32_t>() : nullptr));
    if (keys) HIP_TRY(hipMemcpyAsync(keys, v.gather_keys.p, cnt * 8 * c->KW, hipMemcpyDeviceToHost, s));
    if (counts) HIP_TRY(hipMemcpyAsync(counts, v.gather_counts.p, cnt * 4, hipMemcpyDeviceToHost, s));
    if (other_counts) HIP_TRY(hipMemcpyAsync(other_counts, v.gather_other.p, cnt * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return FK_OK;
}

FK_EXPORT int fk_bin_sizes_range(fk_ctx *c, uint32_t min_count, uint32_t max_count, uint64_t *out) {
    if (!c || !out) return set_err(FK_E_INVALID, "null argument");
    DeviceGuard dg_(c->device);
    FK_TRY(result_ready(c));
    FK_TRY(check_count_range(min_count, max_count));
    return filtered_bin_sizes(c, Filter{min_count, max_count}, out);
}

FK_EXPORT int fk_get_bin_range(fk_ctx *c, int32_t bin, uint32_t min_count, uint32_t max_count, uint64_t *keys,
                               uint32_t *counts, size_t cap, size_t *n) {
    if (!c || !n) return set_err(FK_E_INVALID, "null argument");
    DeviceGuard dg_(c->device);
    FK_TRY(result_ready(c));
    FK_TRY(check_count_range(min_count, max_count));
    return filtered_bin(c, Filter{min_count, max_count}, bin, keys, counts, nullptr, cap, n);
}

FK_EXPORT int fk_write_bins_range(fk_ctx *c, const char *out_dir, uint32_t min_count, uint32_t max_count) {
    if (!c || !out_dir) return set_err(FK_E_INVALID, "null argument");
    DeviceGuard dg_(c->device);
    FK_TRY(result_ready(c));
    FK_TRY(check_count_range(min_count, max_count));
    if (mkdir_p(out_dir) != 0) return set_err(FK_E_IO, "cannot create %s: %s", out_dir, strerror(errno));
    if (c->distinct == 0) return FK_OK;  // no k-mers: no bin files
    Filter f{min_count, max_count};
    DevBuf kept, off, d_off, fkeys, fcounts;
    std::vector<uint64_t> h_off;
    FK_TRY(filtered_offsets(c, f, kept, off, d_off, h_off));
    const uint64_t D = h_off[c->nlb];
    if (D == 0) return FK_OK;  // nothing kept: no bin files
    FK_TRY(ensure(fkeys, D * 8 * c->KW));
    FK_TRY(ensure(fcounts, D * 4));
    FK_TRY(filter_compact(c, f, off.as<uint64_t>(), fkeys.as<uint64_t>(), fcounts.as<uint32_t>(), nullptr));
    // the writer ends with the stream drained (its text copy), before the temporaries are released
    return write_bin_text(c, out_dir, fkeys.as<uint64_t>(), fcounts.as<uint32_t>(), D, d_off.as<uint64_t>(), h_off);
}

FK_EXPORT int fk_bin_sizes_joined(fk_ctx *c, fk_ctx *o, uint32_t min_count, uint32_t max_count, uint32_t other_min,
                                  uint32_t other_max, uint64_t *out) {
    if (!c || !o || !out) return set_err(FK_E_INVALID, "null argument");
    DeviceGuard dg_(c->device);
    FK_TRY(compare_pair(c, o));
    FK_TRY(check_join_range(min_count, max_count, other_min, other_max));
    return filtered_bin_sizes(c, Filter{min_count, max_count, o, other_min, other_max}, out);
}

FK_EXPORT int fk_get_bin_joined(fk_ctx *c, fk_ctx *o, int32_t bin, uint32_t min_count, uint32_t max_count,
                                uint32_t other_min, uint32_t other_max, uint64_t *keys, uint32_t *counts,
                                uint32_t *other_counts, size_t cap, size_t *n) {
    if (!c || !o || !n) return set_err(FK_E_INVALID, "null argument");
    DeviceGuard dg_(c->device);
    FK_TRY(compare_pair(c, o));
    FK_TRY(check_join_range(min_count, max_count, other_min, other_max));
    return filtered_bin(c, Filter{min_count, max_count, o, other_min, other_max}, bin, keys, counts, other_counts, cap, n);
}

// ---------------------------------------------------------------------------
// per-read abundance profiles of the counted result (fk_reads.inc)
// ---------------------------------------------------------------------------

static_assert(FK_READ_TILE == READ_TILE, "fastkmer.h names the kernel's tile");
static_assert(sizeof(fk_read_stat) == 32 && sizeof(ReadStat) == 32, "fk_read_stat is 32 bytes");

// Host only: FASTA / FASTQ text cut into a CSR read batch, the reads as the count sees them.
namespace {
struct CsrOut {
    uint8_t *bases;
    size_t cap_bases;
    uint64_t *offsets;
    size_t cap_reads;
    size_t nr = 0, nb = 0;
    bool fill, over = false;
    void begin_read() {
        if (fill) {
            if (nr < cap_reads)
                offsets[nr] = nb;
            else
                over = true;
        }
        ++nr;
    }
    void append(const uint8_t *p, size_t len) {
        if (fill) {
            if (nb + len <= cap_bases)
                memcpy(bases + nb, p, len);
            else
                over = true;
        }
        nb += len;
    }
};
}  // namespace

FK_EXPORT int fk_reads_csr(const uint8_t *text, size_t n, int32_t format, int32_t min_quality, int32_t quality_offset,
                           uint8_t *bases, size_t cap_bases, uint64_t *offsets, size_t cap_reads, size_t *n_reads,
                           size_t *n_bases) {
    if ((!text && n) || !n_reads || !n_bases) return set_err(FK_E_INVALID, "null argument");
    *n_reads = 0;
    *n_bases = 0;
    if (format != FK_FORMAT_FASTA && format != FK_FORMAT_FASTQ) return set_err(FK_E_INVALID, "unknown input format %d", format);
    if (quality_offset != 33 && quality_offset != 64)
        return set_err(FK_E_INVALID, "quality_offset must be 33 or 64, got %d", quality_offset);
    if (min_quality < 0 || min_quality > 93) return set_err(FK_E_INVALID, "min_quality must be in 0..93, got %d", min_quality);
    CsrOut o{bases, cap_bases, offsets, cap_reads};
    o.fill = bases && offsets;
    uint64_t bad = UINT64_MAX;
    if (format == FK_FORMAT_FASTA) {
        // the parse's grammar (fk_parse.inc, oracle for_each_read): a non-empty line beginning with '>' is a
        // header, the lines up to the next header are its read without their '\n', lines before the first
        // header are no sequence
        bool in_record = false;
        for (size_t pos = 0; pos < n;) {
            const uint8_t *nl = static_cast<const uint8_t *>(memchr(text + pos, '\n', n - pos));
            const size_t e = nl ? (size_t)(nl - text) : n;
            if (e > pos && text[pos] == '>') {
                in_record = true;
                o.begin_read();
            } else if (in_record) {
                o.append(text + pos, e - pos);
            }
            pos = e + 1;
        }
    } else {
        // fk_fastq.inc's grammar: the lines up to the last one holding a byte other than '\n' / '\r', rounded
        // up to whole records of four where blank lines follow; a trailing '\r' is outside the two lengths
        std::vector<size_t> ls;  // line starts, then n + 1 (every line ends one before the next start)
        for (size_t pos = 0; pos < n;) {
            ls.push_back(pos);
            const uint8_t *nl = static_cast<const uint8_t *>(memchr(text + pos, '\n', n - pos));
            pos = nl ? (size_t)(nl - text) + 1 : n + 1;
        }
        const size_t nlines = ls.size();
        ls.push_back(n && text[n - 1] == '\n' ? n : n + 1);
        size_t ntext = 0;  // lines up to the last one with text
        for (size_t i = nlines; i-- > 0 && !ntext;)
            for (size_t q = ls[i]; q + 1 < ls[i + 1]; ++q)
                if (text[q] != '\r') {
                    ntext = i + 1;
                    break;
                }
        const size_t neff = std::min(nlines, (ntext + 3) & ~(size_t)3), nrec = neff / 4;
        if (neff & 3) bad = nrec;
        for (size_t r = 0; r < nrec && r < bad; ++r) {
            const size_t s0 = ls[4 * r], e0 = ls[4 * r + 1] - 1, s1 = ls[4 * r + 1], e1 = ls[4 * r + 2] - 1;
            const size_t s2 = ls[4 * r + 2], e2 = ls[4 * r + 3] - 1, s3 = ls[4 * r + 3], e3 = std::min(ls[4 * r + 4] - 1, n);
            size_t len1 = e1 - s1, len3 = e3 - s3;
            if (len1 && text[e1 - 1] == '\r') --len1;
            if (len3 && text[e3 - 1] == '\r') --len3;
            if (!(e0 > s0 && text[s0] == '@' && e2 > s2 && text[s2] == '+' && len1 == len3)) {
                bad = r;
                break;
            }
            o.begin_read();
            const size_t at = o.nb;
            o.append(text + s1, e1 - s1);
            if (o.fill && !o.over && min_quality > 0)
                for (size_t j = 0; j < len1; ++j)
                    if ((int)text[s3 + j] - quality_offset < min_quality) bases[at + j] = 'N';
        }
    }
    if (o.fill) {
        if (o.nr <= cap_reads)
            offsets[o.nr] = o.nb;
        else
            o.over = true;
    }
    *n_reads = o.nr;
    *n_bases = o.nb;
    if (bad != UINT64_MAX)
        return set_err(FK_E_INVALID, "FASTQ record %llu is malformed (no '@' or '+' line, quality and sequence of "
                                     "different lengths, or the input ends inside it)", (unsigned long long)bad);
    if (o.over)
        return set_err(FK_E_RANGE, "the text holds %zu reads of %zu bases, the buffers hold %zu and %zu", o.nr, o.nb,
                       cap_reads, cap_bases);
    return FK_OK;
}

FK_EXPORT size_t fk_read_stats_scratch_bytes(size_t n_bases) { return 5 * n_bases; }

// offsets[0] == 0 and ascending (host forms)
static int check_offsets(const uint64_t *offsets, size_t n_reads) {
    if (offsets[0] != 0) return set_err(FK_E_INVALID, "offsets[0] is %llu, not 0", (unsigned long long)offsets[0]);
    for (size_t i = 0; i < n_reads; ++i)
        if (offsets[i + 1] < offsets[i])
            return set_err(FK_E_INVALID, "offsets do not ascend at read %zu (%llu after %llu)", i,
                           (unsigned long long)offsets[i + 1], (unsigned long long)offsets[i]);
    return FK_OK;
}

static int need_all_counts(const fk_ctx *c, const char *what) {
    if (c->cfg.n_ranks > 1)
        return set_err(FK_E_INVALID, "%s needs every k-mer's count and this context is rank %d of %d: sum the ranks' "
                                     "fk_read_counts arrays and reduce them with fk_read_stats_of_counts_device",
                       what, c->cfg.rank, c->cfg.n_ranks);
    return FK_OK;
}

FK_EXPORT int fk_read_counts_device(fk_ctx *c, const void *d_bases, const void *d_offsets, size_t n_reads,
                                    void *d_counts, void *d_valid) {
    if (!c) return set_err(FK_E_INVALID, "null ctx");
    DeviceGuard dg_(c->device);
    QueryTables t;
    FK_TRY(query_tables(c, t));
    if (n_reads == 0) return FK_OK;
    if (!d_bases || !d_offsets || !d_counts) return set_err(FK_E_INVALID, "null argument");
    HIP_TRY(launch_read_counts(c->KW, t, static_cast<const uint8_t *>(d_bases), static_cast<const uint64_t *>(d_offsets),
                               n_reads, 0, UINT64_MAX, static_cast<uint32_t *>(d_counts),
                               static_cast<uint8_t *>(d_valid), c->stream));
    return FK_OK;
}

FK_EXPORT int fk_read_counts(fk_ctx *c, const uint8_t *bases, const uint64_t *offsets, size_t n_reads,
                             uint32_t *counts, uint8_t *valid) {
    if (!c) return set_err(FK_E_INVALID, "null ctx");
    DeviceGuard dg_(c->device);
    QueryTables t;
    FK_TRY(query_tables(c, t));
    if (!offsets) return set_err(FK_E_INVALID, "null argument");
    FK_TRY(check_offsets(offsets, n_reads));
    const size_t n = (size_t)offsets[n_reads], k = (size_t)c->cfg.k;
    if (n == 0) return FK_OK;
    if (!bases || !counts) return set_err(FK_E_INVALID, "null argument");
    hipStream_t s = c->stream;
    // positions [at, at + nc) read the bases [at, at + nc + k - 1) and the offsets of the reads that touch them,
    // rebased: the first read cut at `at`, the last at the end of the halo
    const size_t chunk = (size_t)std::min<uint64_t>(query_chunk(), n);
    FK_TRY(ensure(c->vw.q_in, chunk + k));
    FK_TRY(ensure(c->vw.q_counts, (chunk + k) * 4));
    if (valid) FK_TRY(ensure(c->vw.rd_valid, chunk + k));
    std::vector<uint64_t> sub;
    const uint64_t *const oend = offsets + n_reads + 1;
    for (size_t at = 0; at < n; at += chunk) {
        const size_t nc = std::min(chunk, n - at), len = std::min(nc + k - 1, n - at);
        const uint64_t *i0 = std::upper_bound(offsets, oend, (uint64_t)at) - 1;  // the last read beginning at or before
        const uint64_t *i1 = std::lower_bound(i0 + 1, oend, (uint64_t)(at + len));
        const size_t nsub = (size_t)(i1 - i0);
        sub.assign(nsub + 1, 0);
        for (size_t j = 1; j < nsub; ++j) sub[j] = i0[j] - at;
        sub[nsub] = len;
        FK_TRY(ensure(c->vw.rd_off, (nsub + 1) * 8));
        HIP_TRY(hipMemcpyAsync(c->vw.q_in.p, bases + at, len, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(c->vw.rd_off.p, sub.data(), (nsub + 1) * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(launch_read_counts(c->KW, t, c->vw.q_in.as<uint8_t>(), c->vw.rd_off.as<uint64_t>(), nsub, len, len,
                                   c->vw.q_counts.as<uint32_t>(), valid ? c->vw.rd_valid.as<uint8_t>() : nullptr, s));
        HIP_TRY(hipMemcpyAsync(counts + at, c->vw.q_counts.p, nc * 4, hipMemcpyDeviceToHost, s));
        if (valid) HIP_TRY(hipMemcpyAsync(valid + at, c->vw.rd_valid.p, nc, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));  // the staging buffers are free for the next chunk
    }
    return FK_OK;
}

FK_EXPORT int fk_read_stats_of_counts_device(fk_ctx *c, const void *d_counts, const void *d_valid, const void *d_offsets,
                                             size_t n_reads, uint32_t min_count, uint32_t max_count, void *d_stats) {
    if (!c) return set_err(FK_E_INVALID, "null ctx");
    DeviceGuard dg_(c->device);
    FK_TRY(check_count_range(min_count, max_count));
    if (n_reads == 0) return FK_OK;
    if (!d_counts || !d_offsets || !d_stats) return set_err(FK_E_INVALID, "null argument");
    HIP_TRY(launch_read_stats(static_cast<const uint32_t *>(d_counts), static_cast<const uint8_t *>(d_valid),
                              static_cast<const uint64_t *>(d_offsets), n_reads, UINT64_MAX, c->cfg.k, min_count,
                              max_count, static_cast<ReadStat *>(d_stats), c->stream));
    return FK_OK;
}

FK_EXPORT int fk_read_stats_device(fk_ctx *c, const void *d_bases, const void *d_offsets, size_t n_reads,
                                   uint32_t min_count, uint32_t max_count, void *d_scratch, size_t scratch_bytes,
                                   void *d_stats) {
    if (!c) return set_err(FK_E_INVALID, "null ctx");
    DeviceGuard dg_(c->device);
    FK_TRY(need_all_counts(c, "fk_read_stats_device"));
    QueryTables t;
    FK_TRY(query_tables(c, t));
    FK_TRY(check_count_range(min_count, max_count));
    if (n_reads == 0) return FK_OK;
    if (!d_bases || !d_offsets || !d_stats || (!d_scratch && scratch_bytes)) return set_err(FK_E_INVALID, "null argument");
    if (reinterpret_cast<uintptr_t>(d_scratch) & 3) return set_err(FK_E_INVALID, "d_scratch must be 4-byte aligned");
    // the scratch holds uint32 counts then uint8 valid flags of `cap` positions; the kernels stop at cap
    const uint64_t cap = scratch_bytes / 5;
    uint32_t *cnt = static_cast<uint32_t *>(d_scratch);
    uint8_t *val = static_cast<uint8_t *>(d_scratch) + 4 * cap;
    if (cap)
        HIP_TRY(launch_read_counts(c->KW, t, static_cast<const uint8_t *>(d_bases),
                                   static_cast<const uint64_t *>(d_offsets), n_reads, cap, cap, cnt, val, c->stream));
    HIP_TRY(launch_read_stats(cnt, val, static_cast<const uint64_t *>(d_offsets), n_reads, cap, c->cfg.k, min_count,
                              max_count, static_cast<ReadStat *>(d_stats), c->stream));
    return FK_OK;
}

FK_EXPORT int fk_read_stats(fk_ctx *c, const uint8_t *bases, const uint64_t *offsets, size_t n_reads,
                            uint32_t min_count, uint32_t max_count, fk_read_stat *stats) {
    if (!c) return set_err(FK_E_INVALID, "null ctx");
    DeviceGuard dg_(c->device);
    FK_TRY(need_all_counts(c, "fk_read_stats"));
    QueryTables t;
    FK_TRY(query_tables(c, t));
    FK_TRY(check_count_range(min_count, max_count));
    if (!offsets) return set_err(FK_E_INVALID, "null argument");
    FK_TRY(check_offsets(offsets, n_reads));
    if (n_reads == 0) return FK_OK;
    if ((!bases && offsets[n_reads]) || !stats) return set_err(FK_E_INVALID, "null argument");
    hipStream_t s = c->stream;
    // whole reads per chunk: as many as fit FASTKMER_QUERY_CHUNK positions (and as many reads), at least one
    const uint64_t chunk = query_chunk();
    std::vector<uint64_t> sub;
    for (size_t r0 = 0; r0 < n_reads;) {
        size_t r1 = r0 + 1;
        while (r1 < n_reads && offsets[r1 + 1] - offsets[r0] <= chunk && r1 - r0 < chunk) ++r1;
        const size_t nr = r1 - r0, len = (size_t)(offsets[r1] - offsets[r0]);
        sub.resize(nr + 1);
        for (size_t j = 0; j <= nr; ++j) sub[j] = offsets[r0 + j] - offsets[r0];
        FK_TRY(ensure(c->vw.q_in, len));
        FK_TRY(ensure(c->vw.q_counts, len * 4));
        FK_TRY(ensure(c->vw.rd_valid, len));
        FK_TRY(ensure(c->vw.rd_off, (nr + 1) * 8));
        FK_TRY(ensure(c->vw.rd_stats, nr * sizeof(ReadStat)));
        if (len) HIP_TRY(hipMemcpyAsync(c->vw.q_in.p, bases + offsets[r0], len, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(c->vw.rd_off.p, sub.data(), (nr + 1) * 8, hipMemcpyHostToDevice, s));
        if (len)
            HIP_TRY(launch_read_counts(c->KW, t, c->vw.q_in.as<uint8_t>(), c->vw.rd_off.as<uint64_t>(), nr, len, len,
                                       c->vw.q_counts.as<uint32_t>(), c->vw.rd_valid.as<uint8_t>(), s));
        HIP_TRY(launch_read_stats(c->vw.q_counts.as<uint32_t>(), c->vw.rd_valid.as<uint8_t>(), c->vw.rd_off.as<uint64_t>(), nr,
                                  len, c->cfg.k, min_count, max_count, c->vw.rd_stats.as<ReadStat>(), s));
        HIP_TRY(hipMemcpyAsync(stats + r0, c->vw.rd_stats.p, nr * sizeof(ReadStat), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        r0 = r1;
    }
    return FK_OK;
}

