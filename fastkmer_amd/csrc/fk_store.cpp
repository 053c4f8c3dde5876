// fk_store.cpp -- the C-ABI calls that take a counted result out of its context and put one back
// (include/fastkmer.h, "export, import and the database file"): fk_export*, fk_import*, fk_save, fk_load,
// fk_db_info_read.  The kernels are fk_store.inc's and the count's own bucket cut; the file's header is
// fk_db_header.h's.  The result is the context's (fk_ctx.h), bucket-major as the count leaves it.
#include <errno.h>
#include <fcntl.h>
#include <stdio.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <chrono>
#include <cstdlib>

#include "fk_ctx.h"
#include "fk_db_header.h"

namespace {

double wall_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// A call's own timed events.
template <int N>
struct Events {
    Event e[N];
    int create() {
        for (int i = 0; i < N; ++i) HIP_TRY(e[i].create());
        return FK_OK;
    }
    double ms(int a, int b) const {
        float t = 0.f;
        if (hipEventElapsedTime(&t, e[a], e[b]) != hipSuccess) {
            (void)hipGetLastError();
            return 0.0;
        }
        return t;
    }
};

struct Fd {
    int fd = -1;
    ~Fd() {
        if (fd >= 0) close(fd);
    }
};

constexpr size_t STORE_WINDOW = 32ull << 20;  // bytes per pinned window of fk_save / fk_load (file_pin)

int need_sorted_result(const fk_ctx *c) {
    if (c->cfg.use_ht) return set_err(FK_E_INVALID, "%s", MSG_NEED_SORTED);
    if (!c->have_result || (c->distinct && !c->gapped)) return set_err(FK_E_STATE, "no result: call fk_finish or fk_reduce first");
    return FK_OK;
}

// the whole result dense at dk / dc (device), queued on the context's stream
int export_queue(fk_ctx *c, uint64_t *dk, uint32_t *dc) {
    if (c->distinct == 0) return FK_OK;
    HIP_TRY(launch_bucket_compact(c->KW, c->res_keys, c->out_counts.as<uint32_t>(), c->buckets.as<Bucket>(), c->res_nbuckets,
                                  c->dense_off.as<uint64_t>(), dk, dc, c->stream));
    return FK_OK;
}

// The dense arrays' bins in another order: segment i = (source key index, destination key index, keys).
struct Seg {
    uint64_t src, dst, n;
};
int permute_queue(fk_ctx *c, const std::vector<Seg> &segs, const uint64_t *sk, const uint32_t *sc, uint64_t *dk, uint32_t *dc) {
    const size_t kb = (size_t)c->KW * 8;
    for (const Seg &g : segs) {
        HIP_TRY(hipMemcpyAsync(dk + g.dst * c->KW, sk + g.src * c->KW, g.n * kb, hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(dc + g.dst, sc + g.src, g.n * 4, hipMemcpyDeviceToDevice, c->stream));
    }
    return FK_OK;
}

const char *why_text(uint32_t why) {
    switch (why) {
        case STORE_BAD_BITS: return "a bit set above bit 2k - 1";
        case STORE_BAD_STRAND: return "not canonical (greater than its reverse complement)";
        case STORE_BAD_BIN: return "the key's signature puts it in another bin";
        case STORE_BAD_DUP: return "a duplicate of the key before it";
        case STORE_BAD_ORDER: return "not ascending (below the key before it)";
        case STORE_BAD_COUNT: return "count 0";
    }
    return "unknown";
}

// What an import may not interrupt, and the layout of its input: off[0 .. nlb] = the dense offsets of the
// local bins by bin_sizes (all Bc bins).
int import_layout(fk_ctx *c, const uint64_t *bin_sizes, std::vector<uint64_t> &off) {
    if (c->cfg.use_ht) return set_err(FK_E_INVALID, "%s", MSG_NEED_SORTED);
    if (c->job.job_open || c->job.dev_open || c->job.xch.open)
        return set_err(FK_E_STATE, "an import inside a job (between its first fk_ingest and fk_finish)");
    reset_results(c);
    std::vector<uint64_t> per(c->nlb, 0);
    for (int32_t b = 0; b < c->Bc; ++b) {
        if (!bin_sizes[b]) continue;
        if (!owns(c, b))
            return set_err(FK_E_INVALID, "bin %d holds %llu keys and belongs to rank %d, this context is rank %d of %u", b,
                           (unsigned long long)bin_sizes[b], bin_owner(c, b), c->cfg.rank, c->G);
        per[local_bin(c, b)] = bin_sizes[b];
    }
    off.assign((size_t)c->nlb + 1, 0);
    for (uint32_t lb = 0; lb < c->nlb; ++lb) {
        if (per[lb] > (UINT64_MAX >> 8) - off[lb]) return set_err(FK_E_RANGE, "the bins' sizes overflow");
        off[lb + 1] = off[lb] + per[lb];
    }
    return FK_OK;
}

// The import proper.  The keys and counts lie in c->out_keys / c->out_counts (queued on the stream or
// landed), n = off[nlb] of them; import_layout has run.  Queues verify -> cell offsets -> bucket tables,
// waits once, and leaves the context with the result or without one.  sums[0] / [1] = the checksum and
// the sum of the counts.  ev: 4 events around the three steps.
int import_tables(fk_ctx *c, const std::vector<uint64_t> &off, uint64_t sums[2], Events<4> &ev) {
    hipStream_t s = c->stream;
    const uint32_t nlb = c->nlb;
    const uint64_t n = off[nlb];
    const char *tb = getenv("FASTKMER_DEBUG_IMPORT_BUCKET");
    c->import_bucket = tb && tb[0] ? (uint32_t)std::min<unsigned long long>(strtoull(tb, nullptr, 10), 0xffffffffull) : 0u;
    uint64_t max_bin = 0;
    for (uint32_t lb = 0; lb < nlb; ++lb) max_bin = std::max(max_bin, off[lb + 1] - off[lb]);
    const SortedPlan pl = sorted_plan(c, max_bin);
    const int F = pl.F;
    const uint32_t target = c->import_bucket ? c->import_bucket : pl.wave_cap;
    const uint64_t ncell_all = (uint64_t)nlb << F;
    // a bucket per flagged cell at most, whatever the keys are (refused keys give cell totals that mean
    // nothing; the bucket writer must stay inside its array for them too)
    const uint64_t nb_max = ncell_all;
    FK_TRY(ensure(c->bin_off, ((uint64_t)nlb + 1) * 8));
    FK_TRY(ensure(c->misc, 64));
    FK_TRY(ensure(c->cell_base, (ncell_all + 1) * 8));
    FK_TRY(ensure(c->cell_total, ncell_all * 8));
    FK_TRY(ensure(c->flags, ncell_all * 4));
    FK_TRY(ensure(c->flag_scan, (ncell_all + 1) * 8));
    FK_TRY(ensure(c->buckets, nb_max * sizeof(Bucket)));
    FK_TRY(ensure(c->dense_off, (nb_max + 1) * 8));
    // pinned: the bin offsets up, then the verdict, the sums, the cell flag and the buckets' number down
    const size_t up = ((size_t)nlb + 1) * 8;
    if (c->pin_down.ensure(up + 64)) return set_err(FK_E_NOMEM, "hipHostMalloc failed");
    memcpy(c->pin_down.p, off.data(), up);
    uint64_t *down = reinterpret_cast<uint64_t *>(c->pin_down.as<uint8_t>() + up);
    unsigned long long *res = c->misc.as<unsigned long long>();
    HIP_TRY(hipMemcpyAsync(c->bin_off.p, c->pin_down.p, up, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(res, 0, 64, s));
    // 1. verify
    StoreTables t{owner_table(c), local_table(c), c->fm, c->G, (uint32_t)c->cfg.rank, nlb, c->cfg.k, c->cfg.m};
    HIP_TRY(hipEventRecord(ev.e[0], s));
    HIP_TRY(launch_store_verify(c->KW, t, c->out_keys.as<uint64_t>(), c->out_counts.as<uint32_t>(), n,
                                c->bin_off.as<uint64_t>(), res, s));
    HIP_TRY(hipEventRecord(ev.e[1], s));
    // 2. cell offsets (unsorted or misplaced keys give offsets that mean nothing, and stay inside the bin)
    HIP_TRY(launch_store_cells(c->KW, c->out_keys.as<uint64_t>(), c->bin_off.as<uint64_t>(), nlb, c->cfg.k, F,
                               c->cell_base.as<uint64_t>(), c->cell_total.as<uint64_t>(), res, s));
    HIP_TRY(hipEventRecord(ev.e[2], s));
    // 3. bucket tables: the count's greedy cut at `target` keys, its scan and its bucket writer
    HIP_TRY(launch_bucket_flags_greedy(c->cell_total.as<uint64_t>(), nlb, F, target, -1, c->flags.as<uint32_t>(), s));
    HIP_TRY(scan_excl_sum_u32_to_u64(c->flags.as<uint32_t>(), c->flag_scan.as<uint64_t>(), ncell_all,
                                     c->flag_scan.as<uint64_t>() + ncell_all, c->ws, s));
    HIP_TRY(launch_bucket_write(c->cell_base.as<uint64_t>(), c->flags.as<uint32_t>(), c->flag_scan.as<uint64_t>(), nlb, F,
                                nb_max, n, c->buckets.as<Bucket>(), s));
    HIP_TRY(launch_store_finish(c->buckets.as<Bucket>(), c->flag_scan.as<uint64_t>() + ncell_all, nb_max, nlb, F,
                                c->cell_base.as<uint64_t>() + ncell_all, c->dense_off.as<uint64_t>(), s));
    HIP_TRY(hipEventRecord(ev.e[3], s));
    HIP_TRY(hipMemcpyAsync(down, res, 32, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(down + 4, c->flag_scan.as<uint64_t>() + ncell_all, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    c->store_ms[4] = ev.ms(0, 1), c->store_ms[5] = ev.ms(1, 2), c->store_ms[6] = ev.ms(2, 3);
    if (down[0]) {
        const uint64_t code = ~down[0], i = code >> 3;
        const uint32_t lb = (uint32_t)(std::upper_bound(off.begin(), off.end(), i) - off.begin()) - 1;
        return set_err(FK_E_INVALID, "bin %d, key %llu: %s", global_bin(c, std::min(lb, nlb - 1)),
                       (unsigned long long)(i - off[std::min(lb, nlb - 1)]), why_text((uint32_t)(code & 7)));
    }
    if (down[3]) return set_err(FK_E_RANGE, "a cell of the imported result holds 2^32 keys or more");
    const uint64_t nb = down[4];
    if (nb > nb_max) return set_err(FK_E_DEVICE, "the import cut %llu buckets, more than its bound %llu", (unsigned long long)nb,
                                    (unsigned long long)nb_max);
    sums[0] = down[1], sums[1] = down[2];
    c->gapped = true;
    c->dense_ready = false;
    c->res_keys = c->out_keys.as<uint64_t>();
    c->res_fs = c->flag_scan.as<uint64_t>();
    c->res_nbuckets = nb;
    c->res_F = F;
    c->h_bin_off = off;
    c->distinct = n;
    c->distinct_pending = false;
    c->last_np = 0;
    c->stats = fk_stats{};
    c->stats.distinct = n;
    c->stats.kmers = sums[1];
    c->stats.buckets = nb;
    c->stats.fine_bits = (uint64_t)F;
    std::fill(c->tier_last, c->tier_last + 8, 0ull);
    c->have_result = true;
    return FK_OK;
}

int import_arrays(fk_ctx *c, const void *keys, const void *counts, hipMemcpyKind kind, const uint64_t *bin_sizes,
                  uint64_t sums[2]) {
    const double t0 = wall_ms();
    std::fill(c->store_ms, c->store_ms + 8, 0.0);
    std::vector<uint64_t> off;
    FK_TRY(import_layout(c, bin_sizes, off));
    const uint64_t n = off[c->nlb];
    if (n && (!keys || !counts)) return set_err(FK_E_INVALID, "null argument");
    Events<4> ev;
    Events<2> cp;
    FK_TRY(ev.create());
    FK_TRY(cp.create());
    FK_TRY(ensure(c->out_keys, n * 8 * c->KW));
    FK_TRY(ensure(c->out_counts, n * 4));
    HIP_TRY(hipEventRecord(cp.e[0], c->stream));
    if (n) {
        HIP_TRY(hipMemcpyAsync(c->out_keys.p, keys, n * 8 * c->KW, kind, c->stream));
        HIP_TRY(hipMemcpyAsync(c->out_counts.p, counts, n * 4, kind, c->stream));
    }
    HIP_TRY(hipEventRecord(cp.e[1], c->stream));
    const int rc = import_tables(c, off, sums, ev);
    if (rc != FK_OK) {
        (void)hipStreamSynchronize(c->stream);  // the caller's arrays are free on every return
        return rc;
    }
    c->store_ms[1] = cp.ms(0, 1);
    c->store_ms[0] = wall_ms() - t0;
    return FK_OK;
}

// full writes / reads at an offset; false with errno set
bool pwrite_all(int fd, const uint8_t *p, size_t n, uint64_t at) {
    while (n) {
        const ssize_t w = pwrite(fd, p, n, (off_t)at);
        if (w < 0 && errno == EINTR) continue;
        if (w <= 0) return false;
        p += w, n -= (size_t)w, at += (uint64_t)w;
    }
    return true;
}
bool pread_all(int fd, uint8_t *p, size_t n, uint64_t at) {
    while (n) {
        const ssize_t r = pread(fd, p, n, (off_t)at);
        if (r < 0 && errno == EINTR) continue;
        if (r == 0) errno = ENODATA;
        if (r <= 0) return false;
        p += r, n -= (size_t)r, at += (uint64_t)r;
    }
    return true;
}

// The two sections of a file as windows of at most STORE_WINDOW bytes: window j = `bytes` bytes at `dev`
// (device) and at `at` in the file.
struct Window {
    uint8_t *dev;
    uint64_t at;
    size_t bytes;
};
std::vector<Window> section_windows(void *dk, uint64_t key_bytes, void *dc, uint64_t count_bytes, uint64_t at) {
    std::vector<Window> w;
    for (int sec = 0; sec < 2; ++sec) {
        uint8_t *d = static_cast<uint8_t *>(sec ? dc : dk);
        const uint64_t nb = sec ? count_bytes : key_bytes;
        for (uint64_t o = 0; o < nb; o += STORE_WINDOW) w.push_back(Window{d + o, at + o, (size_t)std::min<uint64_t>(STORE_WINDOW, nb - o)});
        at += nb;
    }
    return w;
}

// the non-empty bins ascending with their sizes, and whether that is the dense (local-bin) order
bool stored_order(const fk_ctx *c, const std::vector<uint64_t> &off, std::vector<DbBin> &bins, std::vector<Seg> &segs) {
    bins.clear();
    segs.clear();
    bool same = true;
    uint64_t at = 0;
    for (int32_t b = 0; b < c->Bc; ++b) {
        if (!owns(c, b)) continue;
        const uint32_t lb = local_bin(c, b);
        const uint64_t n = off[lb + 1] - off[lb];
        if (!n) continue;
        bins.push_back(DbBin{(uint32_t)b, n});
        segs.push_back(Seg{off[lb], at, n});  // dense -> stored
        same = same && off[lb] == at;
        at += n;
    }
    return same;
}

}  // namespace

FK_EXPORT int fk_export_device(fk_ctx *c, void *d_keys, void *d_counts, size_t cap, size_t *n) {
    if (!c || !n) return set_err(FK_E_INVALID, "null argument");
    DeviceGuard dg_(c->device);
    *n = 0;
    FK_TRY(need_sorted_result(c));
    *n = (size_t)c->distinct;
    if (cap < c->distinct)
        return set_err(FK_E_RANGE, "the result has %llu k-mers, the buffers hold %zu", (unsigned long long)c->distinct, cap);
    if (c->distinct && (!d_keys || !d_counts)) return set_err(FK_E_INVALID, "null argument");
    return export_queue(c, static_cast<uint64_t *>(d_keys), static_cast<uint32_t *>(d_counts));
}

FK_EXPORT int fk_export(fk_ctx *c, uint64_t *keys, uint32_t *counts, size_t cap, size_t *n) {
    if (!c || !n) return set_err(FK_E_INVALID, "null argument");
    DeviceGuard dg_(c->device);
    *n = 0;
    FK_TRY(need_sorted_result(c));
    const uint64_t D = c->distinct;
    *n = (size_t)D;
    if (cap < D) return set_err(FK_E_RANGE, "the result has %llu k-mers, the buffers hold %zu", (unsigned long long)D, cap);
    if (D == 0) return FK_OK;
    if (!keys || !counts) return set_err(FK_E_INVALID, "null argument");
    DevBuf dk, dc;
    FK_TRY(ensure(dk, D * 8 * c->KW));
    FK_TRY(ensure(dc, D * 4));
    FK_TRY(export_queue(c, dk.as<uint64_t>(), dc.as<uint32_t>()));
    HIP_TRY(hipMemcpyAsync(keys, dk.p, D * 8 * c->KW, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(counts, dc.p, D * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return FK_OK;
}

FK_EXPORT int fk_import_device(fk_ctx *c, const void *d_keys, const void *d_counts, const uint64_t *bin_sizes) {
    if (!c || !bin_sizes) return set_err(FK_E_INVALID, "null argument");
    DeviceGuard dg_(c->device);
    uint64_t sums[2];
    return import_arrays(c, d_keys, d_counts, hipMemcpyDeviceToDevice, bin_sizes, sums);
}

FK_EXPORT int fk_import(fk_ctx *c, const uint64_t *keys, const uint32_t *counts, const uint64_t *bin_sizes) {
    if (!c || !bin_sizes) return set_err(FK_E_INVALID, "null argument");
    DeviceGuard dg_(c->device);
    uint64_t sums[2];
    return import_arrays(c, keys, counts, hipMemcpyHostToDevice, bin_sizes, sums);
}

FK_EXPORT int fk_debug_store_ms(const fk_ctx *c, double out[8]) {
    if (!c || !out) return set_err(FK_E_INVALID, "null argument");
    std::copy(c->store_ms, c->store_ms + 8, out);
    return FK_OK;
}

FK_EXPORT int fk_db_info_read(const char *path, fk_db_info *out) {
    if (!path || !out) return set_err(FK_E_INVALID, "null argument");
    std::string err;
    const int rc = db_read_header(path, out, nullptr, &err);
    return rc == FK_OK ? rc : set_err(rc, "%s", err.c_str());
}

FK_EXPORT int fk_save(fk_ctx *c, const char *path) {
    if (!c || !path) return set_err(FK_E_INVALID, "null argument");
    DeviceGuard dg_(c->device);
    FK_TRY(need_sorted_result(c));
    const double t0 = wall_ms();
    std::fill(c->store_ms, c->store_ms + 8, 0.0);
    hipStream_t s = c->stream;
    const uint64_t D = c->distinct;
    const size_t kb = (size_t)c->KW * 8;
    std::vector<DbBin> bins;
    std::vector<Seg> segs;
    const bool same = stored_order(c, c->h_bin_off, bins, segs);
    Events<4> ev;
    FK_TRY(ev.create());
    // the result dense in the file's order, and its checksum
    DevBuf dk, dc, pk, pc, res;
    FK_TRY(ensure(dk, D * kb));
    FK_TRY(ensure(dc, D * 4));
    FK_TRY(ensure(res, 64));
    HIP_TRY(hipEventRecord(ev.e[0], s));
    FK_TRY(export_queue(c, dk.as<uint64_t>(), dc.as<uint32_t>()));
    uint64_t *fkeys = dk.as<uint64_t>();
    uint32_t *fcounts = dc.as<uint32_t>();
    if (!same) {  // size-aware placement: the local bins are not in ascending bin order
        FK_TRY(ensure(pk, D * kb));
        FK_TRY(ensure(pc, D * 4));
        FK_TRY(permute_queue(c, segs, fkeys, fcounts, pk.as<uint64_t>(), pc.as<uint32_t>()));
        fkeys = pk.as<uint64_t>(), fcounts = pc.as<uint32_t>();
    }
    HIP_TRY(hipMemsetAsync(res.p, 0, 64, s));
    HIP_TRY(launch_store_checksum(fkeys, D * c->KW, fcounts, D, res.as<unsigned long long>(), s));
    HIP_TRY(hipEventRecord(ev.e[1], s));
    uint64_t sums[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(sums, res.p, 32, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    c->store_ms[1] = ev.ms(0, 1);
    fk_db_info h{};
    h.k = c->cfg.k, h.m = c->cfg.m, h.bins = c->Bc, h.key_words = c->KW, h.n_ranks = c->cfg.n_ranks, h.rank = c->cfg.rank;
    h.distinct = D, h.kmers = sums[2], h.checksum = sums[1];
    const std::vector<uint8_t> head = db_build_header(h, bins);

    const std::string tmp = std::string(path) + ".tmp";
    Fd f;
    f.fd = open(tmp.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (f.fd < 0) return set_err(FK_E_IO, "cannot create %s: %s", tmp.c_str(), strerror(errno));
    auto io_fail = [&](const char *what) {
        const int e = errno;
        (void)unlink(tmp.c_str());
        return set_err(FK_E_IO, "%s %s: %s", what, tmp.c_str(), strerror(e));
    };
    if (!pwrite_all(f.fd, head.data(), head.size(), 0)) return io_fail("writing");
    // the sections through the two pinned windows: window j + 1 is copied while window j is written
    const std::vector<Window> w = section_windows(fkeys, D * kb, fcounts, D * 4, head.size());
    for (int b = 0; b < 2 && (size_t)b < w.size(); ++b)
        if (c->file_pin[b].ensure(std::min<uint64_t>(STORE_WINDOW, std::max(D * kb, D * 4))))
            return set_err(FK_E_NOMEM, "hipHostMalloc failed");
    double t_wait = 0.0, t_write = 0.0;
    if (!w.empty()) {
        HIP_TRY(hipMemcpyAsync(c->file_pin[0].p, w[0].dev, w[0].bytes, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipEventRecord(ev.e[2], s));
    }
    for (size_t j = 0; j < w.size(); ++j) {
        const int b = (int)(j & 1);
        if (j + 1 < w.size()) {
            HIP_TRY(hipMemcpyAsync(c->file_pin[b ^ 1].p, w[j + 1].dev, w[j + 1].bytes, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipEventRecord(ev.e[2 + (b ^ 1)], s));
        }
        const double a0 = wall_ms();
        HIP_TRY(hipEventSynchronize(ev.e[2 + b]));
        const double a1 = wall_ms();
        if (!pwrite_all(f.fd, c->file_pin[b].as<uint8_t>(), w[j].bytes, w[j].at)) {
            const int e = errno;
            (void)hipStreamSynchronize(s);  // the copy in flight targets the other window
            errno = e;
            return io_fail("writing");
        }
        t_wait += a1 - a0, t_write += wall_ms() - a1;
    }
    if (close(f.fd) != 0) {
        f.fd = -1;
        return io_fail("closing");
    }
    f.fd = -1;
    if (rename(tmp.c_str(), path) != 0) return io_fail("renaming");
    c->store_ms[2] = t_wait, c->store_ms[3] = t_write;
    c->store_ms[0] = wall_ms() - t0;
    return FK_OK;
}

FK_EXPORT int fk_load(fk_ctx *c, const char *path) {
    if (!c || !path) return set_err(FK_E_INVALID, "null argument");
    DeviceGuard dg_(c->device);
    if (c->cfg.use_ht) return set_err(FK_E_INVALID, "%s", MSG_NEED_SORTED);
    const double t0 = wall_ms();
    std::fill(c->store_ms, c->store_ms + 8, 0.0);
    fk_db_info h;
    std::vector<DbBin> bins;
    std::string err;
    const int prc = db_read_header(path, &h, &bins, &err);
    if (prc != FK_OK) return set_err(prc, "%s", err.c_str());
    if (h.k != c->cfg.k) return set_err(FK_E_INVALID, "%s holds k = %d, the context counts k = %d", path, h.k, c->cfg.k);
    if (h.m != c->cfg.m) return set_err(FK_E_INVALID, "%s holds m = %d, the context has m = %d", path, h.m, c->cfg.m);
    if (h.bins != c->Bc) return set_err(FK_E_INVALID, "%s holds bins = %d, the context has %d", path, h.bins, c->Bc);
    if (h.key_words != c->KW) return set_err(FK_E_INVALID, "%s holds key_words = %d, the context has %d", path, h.key_words, c->KW);
    std::vector<uint64_t> sizes((size_t)c->Bc, 0);
    for (const DbBin &b : bins) {
        if (!owns(c, (int32_t)b.bin))
            return set_err(FK_E_INVALID, "%s (saved by rank %d of %d) holds bin %u, which belongs to rank %d: this context is rank %d of %u",
                           path, h.rank, h.n_ranks, b.bin, bin_owner(c, (int32_t)b.bin), c->cfg.rank, c->G);
        sizes[b.bin] = b.distinct;
    }
    std::vector<uint64_t> off;
    FK_TRY(import_layout(c, sizes.data(), off));
    const uint64_t D = h.distinct;
    const size_t kb = (size_t)c->KW * 8;
    hipStream_t s = c->stream;
    std::vector<DbBin> ord;
    std::vector<Seg> segs;
    const bool same = stored_order(c, off, ord, segs);
    Fd f;
    f.fd = open(path, O_RDONLY);
    if (f.fd < 0) return set_err(FK_E_IO, "cannot open %s: %s", path, strerror(errno));
    Events<4> ev;
    Events<4> cp;
    FK_TRY(ev.create());
    FK_TRY(cp.create());
    FK_TRY(ensure(c->out_keys, D * kb));
    FK_TRY(ensure(c->out_counts, D * 4));
    // the sections land in the context's arrays, or (another order) in temporaries permuted into them
    DevBuf tk, tc;
    uint64_t *fkeys = c->out_keys.as<uint64_t>();
    uint32_t *fcounts = c->out_counts.as<uint32_t>();
    if (!same) {
        FK_TRY(ensure(tk, D * kb));
        FK_TRY(ensure(tc, D * 4));
        fkeys = tk.as<uint64_t>(), fcounts = tc.as<uint32_t>();
    }
    const std::vector<Window> w = section_windows(fkeys, D * kb, fcounts, D * 4, (uint64_t)DB_FIXED + DB_BIN_ENTRY * bins.size());
    for (int b = 0; b < 2 && (size_t)b < w.size(); ++b)
        if (c->file_pin[b].ensure(std::min<uint64_t>(STORE_WINDOW, std::max(D * kb, D * 4))))
            return set_err(FK_E_NOMEM, "hipHostMalloc failed");
    // window j is read while window j - 1 is copied; a window is free again once its copy has landed
    double t_read = 0.0;
    HIP_TRY(hipEventRecord(cp.e[0], s));
    for (size_t j = 0; j < w.size(); ++j) {
        const int b = (int)(j & 1);
        if (j >= 2) HIP_TRY(hipEventSynchronize(cp.e[2 + b]));
        const double a0 = wall_ms();
        if (!pread_all(f.fd, c->file_pin[b].as<uint8_t>(), w[j].bytes, w[j].at)) {
            const int e = errno;
            (void)hipStreamSynchronize(s);
            return set_err(FK_E_IO, "reading %s: %s", path, e == ENODATA ? "truncated" : strerror(e));
        }
        t_read += wall_ms() - a0;
        HIP_TRY(hipMemcpyAsync(w[j].dev, c->file_pin[b].p, w[j].bytes, hipMemcpyHostToDevice, s));
        HIP_TRY(hipEventRecord(cp.e[2 + b], s));
    }
    if (!same) {  // stored -> dense: the segments the other way round
        for (Seg &g : segs) std::swap(g.src, g.dst);
        FK_TRY(permute_queue(c, segs, fkeys, fcounts, c->out_keys.as<uint64_t>(), c->out_counts.as<uint32_t>()));
    }
    HIP_TRY(hipEventRecord(cp.e[1], s));
    uint64_t sums[2] = {0, 0};
    int rc = import_tables(c, off, sums, ev);
    if (rc != FK_OK) (void)hipStreamSynchronize(s);  // before the temporaries and the windows are reused
    if (rc == FK_OK && same && sums[0] != h.checksum)
        rc = set_err(FK_E_INVALID, "%s: checksum mismatch (the file says %016llx, its sections give %016llx)", path,
                     (unsigned long long)h.checksum, (unsigned long long)sums[0]);
    if (rc == FK_OK && sums[1] != h.kmers)
        rc = set_err(FK_E_INVALID, "%s: kmers mismatch (the file says %llu, its counts sum to %llu)", path,
                     (unsigned long long)h.kmers, (unsigned long long)sums[1]);
    if (rc == FK_OK && !same) {
        // the checksum is over the file's order: once more over the sections as they were stored
        DevBuf res;
        uint64_t fs[4] = {0, 0, 0, 0};
        rc = ensure(res, 64);
        if (rc == FK_OK) {
            HIP_TRY(hipMemsetAsync(res.p, 0, 64, s));
            HIP_TRY(launch_store_checksum(fkeys, D * c->KW, fcounts, D, res.as<unsigned long long>(), s));
            HIP_TRY(hipMemcpyAsync(fs, res.p, 32, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            if (fs[1] != h.checksum)
                rc = set_err(FK_E_INVALID, "%s: checksum mismatch (the file says %016llx, its sections give %016llx)", path,
                             (unsigned long long)h.checksum, (unsigned long long)fs[1]);
        }
    }
    if (rc != FK_OK) {
        reset_results(c);
        return rc;
    }
    c->store_ms[1] = cp.ms(0, 1);
    c->store_ms[2] = t_read;
    c->store_ms[0] = wall_ms() - t0;
    return FK_OK;
}
