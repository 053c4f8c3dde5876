// fk_reads.inc: per-read k-mer abundance profiles of the counted result -- included by fk_kernels.hip
// inside namespace fk.
// ---------------------------------------------------------------------------
// 8. read profiles (fk_read_counts*, fk_read_stats*, no reference counterpart).  A read batch is CSR:
//    bases[n_bases] back to back, offsets[n_reads + 1] ascending from 0 to n_bases (on the device:
//    n_bases = offsets[n_reads], so a launch needs no host knowledge of it and its grid is fixed; every
//    workgroup strides over the tiles).
//
//    k_read_counts: window p = bases[p, p + k).  A workgroup takes one tile of READ_TILE positions and
//    their k - 1 halo at a time (its 16 bytes of the next tile are loaded before the lookups of this one):
//      1. stage    16 bytes a thread -> 2-bit codes packed 32 bases to a 64-bit LDS word (first base
//                  highest, so consecutive words read as one long key) and one invalid-byte bit a
//                  position;
//      2. reads    one search in offsets for the first read boundary behind the tile's first position (a
//                  probe a thread and round: three rounds for 2^30 reads), then a walk over the
//                  boundaries inside the staged range: bit q - 1 of the
//                  end-of-read mask for a read ending at q (empty reads repeat a boundary; a read over
//                  many tiles has none inside most of them);
//      3. m-mers   norm_mmer of the m-mer starting at every staged position, once, into LDS; then the
//                  minimum over the w = k - m + 1 values of a window by van Herk / Gil-Werman: prefix
//                  and suffix minima inside blocks of w values, window minimum = min(suffix[p],
//                  prefix[p + w - 1]).  The minimum of norm_mmer over a k-mer's m-mers is kmer_signature
//                  (fk_common.h) bit for bit: its two shifted scans visit the same m-mers and their
//                  reverse complements.  Values of m-mers holding an invalid byte are garbage, and only
//                  invalid windows read them;
//      4. keys     per window two (k <= 32) or three 64-bit LDS words and a funnel shift give the forward
//                  key; reverse complement, canonical key, bin and query_count as in k_query;
//      5. validate k bits of the invalid mask and k - 1 bits of the end-of-read mask from p must be 0.
//    k_read_stats: one wave per read over the position-indexed counts: windows, hits, min, max and sum
//    by wave reductions, the exact median (element (windows - 1) / 2 of the ascending counts) by a
//    32-step bitwise radix select, over registers for reads of at most 256 windows, else re-reading.
// ---------------------------------------------------------------------------

constexpr int RD_NT = 1024;  // one workgroup a CU: 16 waves on one tile (see DESIGN section 4)
constexpr int RS_NT = 256;   // k_read_stats: four reads a workgroup
constexpr int RD_TILE = READ_TILE;
constexpr int RD_STAGE = RD_TILE + 64;      // staged bases: the tile and a k - 1 <= 63 halo, 16-byte units
constexpr int RD_CODE_W = RD_TILE / 32 + 4; // 64-bit words of codes (a window's three words end at word RD_TILE / 32 + 1)
constexpr int RD_MASK_W = RD_TILE / 64 + 2; // 64-bit words of position bits (RD_CODE_W * 2 sixteen-bit units)
constexpr int RD_VALS = RD_TILE + 128;      // m-mer values: RD_TILE + w - 1 rounded up to whole blocks of w <= 64
static_assert(RD_STAGE % 16 == 0 && RD_CODE_W * 2 == RD_MASK_W * 4 && RD_STAGE / 16 <= RD_CODE_W * 2, "staging units");

// n <= 64 bits of a position mask from bit p on
__device__ __forceinline__ uint64_t rd_bits(const uint64_t *w, uint32_t p, int n) {
    const uint32_t j = p >> 6, o = p & 63;
    uint64_t x = w[j] >> o;
    if (o) x |= w[j + 1] << (64 - o);
    return n >= 64 ? x : x & ((1ull << n) - 1ull);
}

template <int KW>
__global__ __launch_bounds__(RD_NT) void k_read_counts(QueryTables t, const uint8_t *__restrict__ bases,
                                                       const uint64_t *__restrict__ offsets, uint64_t n_reads,
                                                       uint64_t cap, uint32_t *__restrict__ counts,
                                                       uint8_t *__restrict__ valid) {
    __shared__ uint64_t s_code[RD_CODE_W];
    __shared__ uint64_t s_inv[RD_MASK_W], s_end[RD_MASK_W];
    __shared__ uint32_t s_v[RD_VALS], s_pre[RD_VALS];
    const int tid = threadIdx.x;
    const int k = t.k, m = t.m, w = k - m + 1;
    const uint32_t def = 1u << (2 * m);
    uint64_t n_bases = offsets[n_reads];
    if (n_bases > cap) n_bases = cap;
    uint32_t *const code32 = reinterpret_cast<uint32_t *>(s_code);
    uint16_t *const inv16 = reinterpret_cast<uint16_t *>(s_inv);
    uint32_t *const end32 = reinterpret_cast<uint32_t *>(s_end);
    const bool aligned = (reinterpret_cast<uintptr_t>(bases) & 15) == 0;

    // the 16 bases thread tid stages of the tile at t0 (zero bytes past the end: invalid positions)
    auto load_unit = [&](uint64_t t0) {
        uint4 q = make_uint4(0, 0, 0, 0);
        const uint64_t g = t0 + 16ull * tid;
        if (tid < RD_STAGE / 16 && g < n_bases) {
            if (aligned && g + 16 <= n_bases) {
                q = *reinterpret_cast<const uint4 *>(bases + g);
            } else {
                for (int j = 0; j < 16 && g + j < n_bases; ++j) {
                    const uint32_t b = (uint32_t)bases[g + j] << (8 * (j & 3));
                    if (j < 4)
                        q.x |= b;
                    else if (j < 8)
                        q.y |= b;
                    else if (j < 12)
                        q.z |= b;
                    else
                        q.w |= b;
                }
            }
        }
        return q;
    };

    const uint64_t stride = (uint64_t)gridDim.x * RD_TILE;
    uint64_t t0 = (uint64_t)blockIdx.x * RD_TILE;
    uint4 q = t0 < n_bases ? load_unit(t0) : make_uint4(0, 0, 0, 0);
    for (; t0 < n_bases; t0 += stride) {
        // 1. stage: unit h = bases [t0 + 16 h, t0 + 16 h + 16), loaded a tile ahead
        if (tid < RD_CODE_W * 2) {
            const int h = tid;
            uint32_t codes = 0, inv = 0;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const uint32_t word = j < 4 ? q.x : j < 8 ? q.y : j < 12 ? q.z : q.w;
                const uint32_t c = base_code((uint8_t)(word >> (8 * (j & 3))));
                codes = (codes << 2) | (c & 3u);
                inv |= (c >> 2) << j;
            }
            code32[h ^ 1] = codes;  // the earlier 16 bases are the high half of their 64-bit word
            inv16[h] = (uint16_t)inv;
        }
        if (tid < RD_MASK_W * 2) end32[tid] = 0;
        __syncthreads();

        // 2. read boundaries q = offsets[i], 1 <= i <= n_reads, with t0 < q <= t0 + RD_STAGE: the first by a
        //    search with one probe a thread and round (the probes ascend, so the count of those at or below
        //    t0 names the interval), the others by a walk
        {
            uint64_t lo = 1, hi = n_reads + 1;  // the first i in [lo, hi) with offsets[i] > t0; hi when none
            while (lo < hi) {
                const uint64_t step = (hi - lo + RD_NT - 1) / RD_NT, idx = lo + (uint64_t)tid * step;
                const uint64_t c = (uint64_t)__syncthreads_count(idx < hi && offsets[idx] <= t0);
                const uint64_t nhi = min<uint64_t>(lo + c * step, hi);
                if (c) lo += (c - 1) * step + 1;
                hi = nhi;
            }
            for (uint64_t i = lo + tid;; i += RD_NT) {
                bool in = i <= n_reads;
                if (in) {
                    const uint64_t e = offsets[i];
                    in = e <= t0 + RD_STAGE;
                    if (in) {
                        const uint32_t bit = (uint32_t)(e - 1 - t0);
                        atomicOr(&end32[bit >> 5], 1u << (bit & 31));
                    }
                }
                if (!__syncthreads_and(in)) break;  // ascending: the first boundary outside ends the walk
            }
        }

        // 3. the m-mer value of every staged position, then block prefix / suffix minima
        const int nv = RD_TILE + w - 1, nseg = (nv + w - 1) / w;
        for (int p = tid; p < nseg * w; p += RD_NT) {
            uint32_t v = def;
            if (p < nv) {
                const uint32_t j = (uint32_t)p >> 5, o = (uint32_t)p & 31;
                const u128 x = (((u128)s_code[j] << 64) | s_code[j + 1]) << (2 * o);
                v = norm_mmer((uint32_t)(x >> (128 - 2 * m)), m);
            }
            s_v[p] = v;
        }
        __syncthreads();
        if (w > 1) {
            for (int seg = tid; seg < nseg; seg += RD_NT) {
                const int b0 = seg * w;
                uint32_t run = def;
                for (int j = 0; j < w; ++j) {
                    run = min(run, s_v[b0 + j]);
                    s_pre[b0 + j] = run;
                }
                run = def;
                for (int j = w - 1; j >= 0; --j) {
                    run = min(run, s_v[b0 + j]);
                    s_v[b0 + j] = run;  // suffix minima replace the values
                }
            }
            __syncthreads();
        }

        if (t0 + stride < n_bases) q = load_unit(t0 + stride);  // in flight during the lookups

        // 4. + 5. one window per lane and pass
        for (int p = tid; p < RD_TILE && t0 + p < n_bases; p += RD_NT) {
            const bool ok = rd_bits(s_inv, (uint32_t)p, k) == 0 && rd_bits(s_end, (uint32_t)p, k - 1) == 0;
            uint32_t cnt = 0;
            if (ok) {
                const uint32_t j = (uint32_t)p >> 5, o = (uint32_t)p & 31;
                u128 x = ((u128)s_code[j] << 64) | s_code[j + 1];
                if (o) {
                    x <<= 2 * o;
                    if constexpr (KW == 2) x |= (u128)(s_code[j + 2] >> (64 - 2 * o));
                }
                x >>= 128 - 2 * k;
                const KmerKey f{KW == 2 ? (uint64_t)(x >> 64) : 0ull, (uint64_t)x};
                const KmerKey r = revcomp_key<KW == 2>(f, k);
                const uint32_t sig = w > 1 ? min(s_v[p], s_pre[p + w - 1]) : s_v[p];
                cnt = query_count<KW>(t, key_less(r, f) ? r : f, bin_of_signature(sig, t.fm));
            }
            counts[t0 + p] = cnt;
            if (valid) valid[t0 + p] = ok ? 1 : 0;
        }
        __syncthreads();  // the next tile restages
    }
}

// The grid: every workgroup strides over the tiles, one workgroup a CU (fewer when the host knows an upper
// bound of n_bases: positions, else 0).  A CU's lookups then all belong to one tile's few dozen reads and share
// their bins' tables in its caches; two workgroups a CU measured a fifth slower (DESIGN section 4).
static hipError_t read_counts_grid(uint64_t positions, unsigned *grid) {
    static int cus = 0;  // per process: the devices of a job are alike
    if (!cus) {
        int dev = 0, n = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e == hipSuccess) e = hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
        if (e != hipSuccess) return e;
        cus = std::max(n, 1);
    }
    *grid = (unsigned)cus;
    if (positions) *grid = (unsigned)std::min<uint64_t>((positions + RD_TILE - 1) / RD_TILE, *grid);
    return hipSuccess;
}

hipError_t launch_read_counts(int KW, const QueryTables &t, const uint8_t *bases, const uint64_t *offsets,
                              uint64_t n_reads, uint64_t positions, uint64_t cap, uint32_t *counts, uint8_t *valid,
                              hipStream_t s) {
    unsigned grid = 1;
    const hipError_t e = read_counts_grid(positions, &grid);
    if (e != hipSuccess) return e;
    if (KW == 1)
        k_read_counts<1><<<grid, RD_NT, 0, s>>>(t, bases, offsets, n_reads, cap, counts, valid);
    else
        k_read_counts<2><<<grid, RD_NT, 0, s>>>(t, bases, offsets, n_reads, cap, counts, valid);
    return hipGetLastError();
}

constexpr int RS_REG = 4;  // windows a lane keeps in registers: reads of up to 64 * RS_REG windows

template <typename T, class F>
__device__ __forceinline__ T wave_all(T v, F op) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = op(v, (T)__shfl_xor(v, d, 64));
    return v;
}

__global__ __launch_bounds__(RS_NT) void k_read_stats(const uint32_t *__restrict__ counts,
                                                      const uint8_t *__restrict__ valid,
                                                      const uint64_t *__restrict__ offsets, uint64_t n_reads, uint64_t cap,
                                                      int k, uint32_t lo, uint32_t hi, ReadStat *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const uint64_t r = (uint64_t)blockIdx.x * (RS_NT / 64) + (threadIdx.x >> 6);
    if (r >= n_reads) return;
    const uint64_t b = offsets[r], len = offsets[r + 1] - b;
    const uint64_t nw = len >= (uint64_t)k ? len - k + 1 : 0;
    uint32_t c[RS_REG], vm = 0;
    uint32_t windows = 0, hits = 0, mn = 0xffffffffu, mx = 0;
    uint64_t sum = 0;
    auto take = [&](bool ok, uint32_t x) {
        windows += ok;
        hits += ok && x >= lo && x <= hi;
        if (ok) mn = min(mn, x), mx = max(mx, x);
        sum += x;
    };
#pragma unroll
    for (int s = 0; s < RS_REG; ++s) {
        const uint64_t i = (uint64_t)lane + 64u * s;
        const bool ok = i < nw && b + i < cap && (!valid || valid[b + i]);
        c[s] = ok ? counts[b + i] : 0u;
        vm |= (uint32_t)ok << s;
        take(ok, c[s]);
    }
    for (uint64_t base = 64u * RS_REG; base < nw; base += 64) {
        const uint64_t i = base + lane;
        const bool ok = i < nw && b + i < cap && (!valid || valid[b + i]);
        take(ok, ok ? counts[b + i] : 0u);
    }
    windows = wave_all(windows, [](uint32_t x, uint32_t y) { return x + y; });
    hits = wave_all(hits, [](uint32_t x, uint32_t y) { return x + y; });
    mn = wave_all(mn, [](uint32_t x, uint32_t y) { return x < y ? x : y; });
    mx = wave_all(mx, [](uint32_t x, uint32_t y) { return x > y ? x : y; });
    sum = wave_all(sum, [](uint64_t x, uint64_t y) { return x + y; });

    uint32_t med = mn;
    if (windows && mn != mx) {
        // the value of rank `rank` among the valid counts, bit by bit from the top: of the values that
        // share the bits chosen so far, n0 have a 0 in this bit
        uint32_t rank = (windows - 1) / 2, prefix = 0;
        for (int bit = 31; bit >= 0; --bit) {
            const uint32_t himask = bit == 31 ? 0u : ~0u << (bit + 1);
            uint32_t n0 = 0;
#pragma unroll
            for (int s = 0; s < RS_REG; ++s)
                n0 += __popcll(__ballot(((vm >> s) & 1u) && (c[s] & himask) == prefix && !((c[s] >> bit) & 1u)));
            for (uint64_t base = 64u * RS_REG; base < nw; base += 64) {
                const uint64_t i = base + lane;
                const bool ok = i < nw && b + i < cap && (!valid || valid[b + i]);
                const uint32_t x = ok ? counts[b + i] : 0u;
                n0 += __popcll(__ballot(ok && (x & himask) == prefix && !((x >> bit) & 1u)));
            }
            if (rank >= n0) {
                rank -= n0;
                prefix |= 1u << bit;
            }
        }
        med = prefix;
    }
    if (lane == 0) {
        ReadStat st;
        st.windows = windows;
        st.hits = hits;
        st.min = windows ? mn : 0u;
        st.median = windows ? med : 0u;
        st.max = mx;
        st.reserved = 0;
        st.sum = sum;
        out[r] = st;
    }
}

hipError_t launch_read_stats(const uint32_t *counts, const uint8_t *valid, const uint64_t *offsets, uint64_t n_reads,
                             uint64_t cap, int k, uint32_t lo, uint32_t hi, ReadStat *out, hipStream_t s) {
    if (!n_reads) return hipSuccess;
    const uint64_t nb = (n_reads + RS_NT / 64 - 1) / (RS_NT / 64);
    if (nb > 0x7fffffffull) return hipErrorInvalidValue;
    k_read_stats<<<(unsigned)nb, RS_NT, 0, s>>>(counts, valid, offsets, n_reads, cap, k, lo, hi, out);
    return hipGetLastError();
}
