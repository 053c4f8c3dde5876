// fk_spectrum.inc: abundance spectrum and count-range views of the counted result -- included by
// fk_kernels.hip inside namespace fk.
// ---------------------------------------------------------------------------
// 8. spectrum and count ranges (fk_spectrum*, fk_*_range, no reference counterpart; their host side
//    is fk_views.cpp).  Both count modes leave the result bucket-major (the count's sorted_result,
//    fk_api.cpp): bucket q's distinct keys at
//    res_keys + KW * buckets[q].begin, their counts at out_counts + buckets[q].begin,
//    dense_off[q + 1] - dense_off[q] of them; use_ht only changes the order inside a bucket.  The
//    arrays have gaps (a bucket's slots are its keys, not its distinct keys), so every kernel
//    here walks bucket by bucket, one wave per bucket in 64-wide strips, as k_bucket_compact does.
//
//    Spectrum: only the counts are read (4 bytes per distinct k-mer, plus 24 bytes of bucket
//    metadata per bucket).  Sequencing data is skewed -- most distinct k-mers occur once -- so one
//    atomic per lane would serialise on hist[1].  A wave therefore
//      - counts the k-mers with count 1 .. SPEC_WAVE in per-lane registers (a compare and an add
//        per strip, no atomic; summed over the wave once, at the end): where the error k-mers are.
//        Ballot + popcount into wave-uniform accumulators gives the same sums and measured slower
//        (113 us against 99 at the job of profiles/spectrum_rate.txt, 17 cycles per ballot),
//      - keeps the last entry (count >= n - 1) and its k-mer sum in per-lane registers,
//      - adds the other counts below SPEC_LDS to a workgroup-private LDS table, one LDS atomic per
//        lane (a coverage peak spreads over tens of entries: few lanes share one),
//      - sends counts >= SPEC_LDS (and below n - 1) to device-scope global atomics: rare.
//    The grid is persistent (it strides the buckets), so a workgroup flushes its table once, the
//    nonzero entries only.  LDS entries and lane counters are 32-bit when the result holds fewer
//    than 2^32 k-mers (each adds 1 per k-mer), else 64-bit.
// ---------------------------------------------------------------------------

constexpr uint32_t SPEC_LDS = 1024;   // counts below this go to the workgroup's LDS table (4 KB, or 8)
constexpr unsigned SPEC_GRID = 2048;  // persistent grid: 8 workgroups per CU
constexpr int SPEC_STRIPS = 4;        // 64-count strips a wave loads before it bins them
// counts 1 .. SPEC_WAVE are summed in per-lane registers (2: 99 us at the configs[1]-parameter job of
// profiles/spectrum_rate.txt; 0: 166, 4: 107, 8: 130)
constexpr uint32_t SPEC_WAVE = 2;
static_assert(SPEC_WAVE < SPEC_LDS && SPEC_WAVE < NT, "the register counts are LDS table entries too");

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += (uint64_t)__shfl_xor(v, d, 64);
    return v;
}

// hist / tail zeroed by the launcher; last = n - 1 >= 1; counts holds at least one entry.  LT: the LDS
// table's entries and the per-lane counters, 32-bit when the whole result holds fewer than 2^32 k-mers
// (a lane adds 1 per k-mer, so none can wrap), else 64-bit.  WAVE: counts 1 .. WAVE stay in registers.
template <typename LT, uint32_t WAVE>
__global__ __launch_bounds__(NT) void k_spectrum(const uint32_t *__restrict__ counts,
                                                 const Bucket *__restrict__ buckets,
                                                 const uint64_t *__restrict__ dense_off, uint64_t nbuckets,
                                                 unsigned long long *__restrict__ hist, uint64_t last,
                                                 unsigned long long *__restrict__ tail) {
    __shared__ LT s_hist[SPEC_LDS];
    __shared__ unsigned long long s_low[WAVE + 1];  // the waves' register counters summed, counts 1 .. WAVE
    __shared__ unsigned long long s_tail[2];
    for (uint32_t i = threadIdx.x; i < SPEC_LDS; i += NT) s_hist[i] = 0;
    if (threadIdx.x <= WAVE) s_low[threadIdx.x] = 0ull;
    if (threadIdx.x < 2) s_tail[threadIdx.x] = 0ull;
    __syncthreads();
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const uint64_t stride = (uint64_t)gridDim.x * (NT / 64);
    // per lane: k-mers seen with count v; dropped at the end when v >= last (those are the tail's: no
    // branch per count in the strip loop).  LT is wide enough for them as for the LDS entries.
    LT acc[WAVE + 1] = {};
    uint64_t tail_n = 0, tail_sum = 0; // per lane
    // A bucket costs two dependent round trips (its metadata, then its counts) of a few 256-B loads,
    // so a wave keeps three buckets in flight: it bins bucket q while the first SPEC_STRIPS strips of
    // bucket q + stride and the metadata of bucket q + 2 stride are on their way.  For that the loads
    // are unconditional (a bucket past the end reads the last bucket's metadata and takes no keys, a
    // lane past a bucket's end reads counts[0]; both are dropped when the strip is binned) and the
    // two strip buffers swap roles instead of being copied: a branch or a copy would make the wave
    // wait for everything in flight.
    const auto meta = [&](uint64_t b, uint64_t &src, uint64_t &nu) {
        const uint64_t bb = b < nbuckets ? b : nbuckets - 1;
        src = buckets[bb].begin;
        const uint64_t d = dense_off[bb + 1] - dense_off[bb];
        nu = b < nbuckets ? d : 0;
    };
    // the counts [i, i + 64 SPEC_STRIPS) of a bucket: `rem` of them exist (0 .. 64 SPEC_STRIPS), the
    // addresses are a wave-uniform base plus a 32-bit lane offset
    constexpr uint32_t SPAN = 64 * SPEC_STRIPS;
    const auto span = [](uint64_t nu, uint64_t i) { return (uint32_t)(nu - i < SPAN ? nu - i : SPAN); };
    const auto load = [&](uint64_t src, uint64_t nu, uint64_t i, uint32_t(&cs)[SPEC_STRIPS]) {
        const uint32_t rem = span(nu, i);
        const uint32_t *__restrict__ p = rem ? counts + src + i : counts;
#pragma unroll
        for (int j = 0; j < SPEC_STRIPS; ++j) {
            const uint32_t r = 64u * j + (uint32_t)lane;
            cs[j] = p[r < rem ? r : 0u];
        }
    };
    const auto bin = [&](const uint32_t(&cs)[SPEC_STRIPS], uint64_t nu, uint64_t i) {
        const uint32_t rem = span(nu, i);
#pragma unroll
        for (int j = 0; j < SPEC_STRIPS; ++j) {
            const uint32_t c = 64u * j + (uint32_t)lane < rem ? cs[j] : 0u;  // no k-mer of a result has count 0
            const bool is_tail = c >= last;  // last >= 1
            if (is_tail) {
                tail_n += 1;
                tail_sum += c;
            }
#pragma unroll
            for (uint32_t v = 1; v <= WAVE; ++v) acc[v] += (LT)(c == v);
            if (c > WAVE && !is_tail) {
                if (c < SPEC_LDS)
                    atomicAdd(&s_hist[c], (LT)1);
                else
                    atomicAdd(&hist[c], 1ull);
            }
        }
    };
    uint64_t q = (uint64_t)blockIdx.x * (NT / 64) + wid;
    uint64_t src, nu, src_n, nu_n;
    uint32_t ca[SPEC_STRIPS], cb[SPEC_STRIPS];
    meta(q, src, nu);
    meta(q + stride, src_n, nu_n);
    load(src, nu, 0, ca);
    // bucket q's first strips are in `cur`; the next bucket's go to `nxt`
    const auto step = [&](uint32_t(&cur)[SPEC_STRIPS], uint32_t(&nxt)[SPEC_STRIPS]) {
        uint64_t src_nn, nu_nn;
        load(src_n, nu_n, 0, nxt);
        meta(q + 2 * stride, src_nn, nu_nn);
        bin(cur, nu, 0);
        for (uint64_t i = 64 * SPEC_STRIPS; i < nu; i += 64 * SPEC_STRIPS) {  // a long bucket's other strips
            load(src, nu, i, cur);
            bin(cur, nu, i);
        }
        q += stride;
        src = src_n, nu = nu_n;
        src_n = src_nn, nu_n = nu_nn;
    };
    while (q < nbuckets) {
        step(ca, cb);
        if (q >= nbuckets) break;
        step(cb, ca);
    }
    tail_n = wave_sum_u64(tail_n);
    tail_sum = wave_sum_u64(tail_sum);
#pragma unroll
    for (uint32_t v = 1; v <= WAVE; ++v) {
        const uint64_t a = wave_sum_u64((uint64_t)acc[v]);
        if (lane == 0 && a && v < last) atomicAdd(&s_low[v], (unsigned long long)a);
    }
    if (lane == 0) {
        if (tail_n) {
            atomicAdd(&s_tail[0], (unsigned long long)tail_n);
            atomicAdd(&s_tail[1], (unsigned long long)tail_sum);
        }
    }
    __syncthreads();
    // entries at or above `last` were never added to (those counts went to the tail)
    for (uint32_t i = threadIdx.x; i < SPEC_LDS; i += NT) {
        const unsigned long long v = (unsigned long long)s_hist[i] + (i <= WAVE ? s_low[i] : 0ull);
        if (v && i < last) atomicAdd(&hist[i], v);
    }
    if (threadIdx.x == 0 && s_tail[0]) {
        atomicAdd(&hist[last], s_tail[0]);
        if (tail) atomicAdd(tail, s_tail[1]);
    }
}

hipError_t launch_spectrum(const uint32_t *counts, const Bucket *buckets, const uint64_t *dense_off,
                           uint64_t nbuckets, uint64_t distinct, uint64_t *hist, uint64_t n, uint64_t *tail,
                           hipStream_t s) {
    if (n < 2) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(hist, 0, n * 8, s);
    if (e == hipSuccess && tail) e = hipMemsetAsync(tail, 0, 8, s);
    if (e != hipSuccess || !nbuckets) return e;
    const unsigned grid = (unsigned)std::min<uint64_t>((nbuckets + NT / 64 - 1) / (NT / 64), SPEC_GRID);
    unsigned long long *h = reinterpret_cast<unsigned long long *>(hist), *t = reinterpret_cast<unsigned long long *>(tail);
    if (distinct >> 32)
        k_spectrum<unsigned long long, SPEC_WAVE><<<grid, NT, 0, s>>>(counts, buckets, dense_off, nbuckets, h, n - 1, t);
    else
        k_spectrum<uint32_t, SPEC_WAVE><<<grid, NT, 0, s>>>(counts, buckets, dense_off, nbuckets, h, n - 1, t);
    return hipGetLastError();
}

// ---- count ranges: a k-mer is kept when lo <= count <= hi

// kept[q] = kept k-mers of bucket q, one wave per bucket
__global__ __launch_bounds__(NT) void k_range_count(const uint32_t *__restrict__ counts,
                                                    const Bucket *__restrict__ buckets,
                                                    const uint64_t *__restrict__ dense_off, uint64_t nbuckets,
                                                    uint32_t lo, uint32_t hi, uint64_t *__restrict__ kept) {
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const uint64_t stride = (uint64_t)gridDim.x * (NT / 64);
    for (uint64_t q = (uint64_t)blockIdx.x * (NT / 64) + wid; q < nbuckets; q += stride) {
        const uint64_t src = buckets[q].begin;
        const uint64_t nu = dense_off[q + 1] - dense_off[q];
        uint64_t cnt = 0;  // wave-uniform
        for (uint64_t i = 0; i < nu; i += 64) {
            const bool valid = i + lane < nu;
            const uint32_t c = valid ? counts[src + i + lane] : 0u;
            cnt += (uint64_t)__popcll(__ballot(valid && c >= lo && c <= hi));
        }
        if (lane == 0) kept[q] = cnt;
    }
}

// bucket q's kept k-mers, in the bucket's order, at keep_off[q] of the dense filtered arrays: the
// place inside a strip is the ballot's bits below the lane, the strips share a running base
template <int KW>
__global__ __launch_bounds__(NT) void k_range_compact(const uint64_t *__restrict__ out_keys,
                                                      const uint32_t *__restrict__ out_counts,
                                                      const Bucket *__restrict__ buckets,
                                                      const uint64_t *__restrict__ dense_off,
                                                      const uint64_t *__restrict__ keep_off, uint64_t nbuckets,
                                                      uint32_t lo, uint32_t hi, uint64_t *__restrict__ fkeys,
                                                      uint32_t *__restrict__ fcounts) {
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const uint64_t stride = (uint64_t)gridDim.x * (NT / 64);
    const uint64_t below = (1ull << lane) - 1ull;
    for (uint64_t q = (uint64_t)blockIdx.x * (NT / 64) + wid; q < nbuckets; q += stride) {
        uint64_t base = keep_off[q];
        if (keep_off[q + 1] == base) continue;  // nothing kept (the singletons-only buckets)
        const uint64_t src = buckets[q].begin;
        const uint64_t nu = dense_off[q + 1] - dense_off[q];
        for (uint64_t i = 0; i < nu; i += 64) {
            const bool valid = i + lane < nu;
            const uint32_t c = valid ? out_counts[src + i + lane] : 0u;
            const bool keep = valid && c >= lo && c <= hi;
            const uint64_t mask = __ballot(keep);
            if (keep) {
                const uint64_t d = base + (uint64_t)__popcll(mask & below);
                if constexpr (KW == 1) {
                    fkeys[d] = out_keys[src + i + lane];
                } else {
                    fkeys[2 * d] = out_keys[2 * (src + i + lane)];
                    fkeys[2 * d + 1] = out_keys[2 * (src + i + lane) + 1];
                }
                fcounts[d] = c;
            }
            base += (uint64_t)__popcll(mask);
        }
    }
}

static unsigned range_grid(uint64_t nbuckets) {
    // one wave per bucket, as k_bucket_compact: the metadata loads are a dependent round trip
    return (unsigned)std::min<uint64_t>((nbuckets + NT / 64 - 1) / (NT / 64), 0x7fffffffull);
}

hipError_t launch_range_count(const uint32_t *counts, const Bucket *buckets, const uint64_t *dense_off,
                              uint64_t nbuckets, uint32_t lo, uint32_t hi, uint64_t *kept, hipStream_t s) {
    if (!nbuckets) return hipSuccess;
    k_range_count<<<range_grid(nbuckets), NT, 0, s>>>(counts, buckets, dense_off, nbuckets, lo, hi, kept);
    return hipGetLastError();
}

hipError_t launch_range_compact(int KW, const uint64_t *out_keys, const uint32_t *out_counts, const Bucket *buckets,
                                const uint64_t *dense_off, const uint64_t *keep_off, uint64_t nbuckets, uint32_t lo,
                                uint32_t hi, uint64_t *fkeys, uint32_t *fcounts, hipStream_t s) {
    if (!nbuckets) return hipSuccess;
    if (KW == 1)
        k_range_compact<1><<<range_grid(nbuckets), NT, 0, s>>>(out_keys, out_counts, buckets, dense_off, keep_off,
                                                               nbuckets, lo, hi, fkeys, fcounts);
    else
        k_range_compact<2><<<range_grid(nbuckets), NT, 0, s>>>(out_keys, out_counts, buckets, dense_off, keep_off,
                                                               nbuckets, lo, hi, fkeys, fcounts);
    return hipGetLastError();
}
