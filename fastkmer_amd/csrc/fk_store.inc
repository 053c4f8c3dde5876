// fk_store.inc: a result built from sorted keys and counts, and the database checksum -- included by
// fk_kernels.hip inside namespace fk.
// ---------------------------------------------------------------------------
// 8. import / export (fk_import*, fk_export*, fk_save, fk_load; no reference counterpart; their host
//    side is fk_store.cpp).  The export is launch_bucket_compact over every bucket.  The import takes
//    the dense arrays the export gives -- every local bin's distinct keys ascending, the bins back to
//    back at bin_off[0 .. nlb] -- and rebuilds the tables fk_query.inc reads, without gaps:
//    buckets[q].begin == dense_off[q].
//      k_store_verify   one lane per key: a k-mer, canonical, in the bin its position says, above its
//                       predecessor, count >= 1; the smallest offending index and its reason, the
//                       checksum of the file format and the sum of the counts
//      k_store_cells    one lane per (local bin, cell): the cell's first key by binary search in the
//                       bin's ascending keys -> cell_base, the exclusive scan the bucket cut reads
//      k_store_cell_totals, then the count's own k_bucket_flags_greedy / scan / k_bucket_write
//      k_store_finish   every bucket's n and c1 from the next bucket, dense_off[q] = begin; the number
//                       of buckets is read on the device (flag_scan's last word): the host waits once
//    The keys' pass has no atomics; the verdict and the sums take one atomic per wave / workgroup.
// ---------------------------------------------------------------------------

// splitmix64's finaliser (fk_common.h's splitmix64 without the increment)
FK_HD uint64_t store_mix(uint64_t x) {
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
    x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}
// one term of the checksum: value v at index i of its section (counts: i = 2^63 + the count's index)
FK_HD uint64_t store_term(uint64_t v, uint64_t i) { return store_mix(v ^ (i * 0x9e3779b97f4a7c15ull)); }

constexpr int STORE_GRID_MAX = 2048;  // workgroups of the grid-stride passes (256 CUs x 8)

// The largest lb in [lo, hi] with off[lb] <= i: the local bin of dense index i when off[hi + 1] > i
// (an empty bin shares its offset with its successor and is never the largest).
__device__ __forceinline__ uint32_t store_bin_of(const uint64_t *__restrict__ off, uint32_t lo, uint32_t hi, uint64_t i) {
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo + 1) >> 1);
        if (off[mid] <= i)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// res[0] = max over the offending keys of ~((index << 3) | reason), 0: none (the smallest index wins,
// and of its reasons the first checked); res[1] += the checksum's terms; res[2] += the counts
template <int KW>
__global__ __launch_bounds__(NT) void k_store_verify(StoreTables t, const uint64_t *__restrict__ keys,
                                                     const uint32_t *__restrict__ counts, uint64_t n,
                                                     const uint64_t *__restrict__ bin_off,
                                                     unsigned long long *__restrict__ res) {
    __shared__ uint64_t s_sum[2][NT / 64];
    const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint64_t bad = 0, sum = 0, kmers = 0;
    for (uint64_t base = (uint64_t)blockIdx.x * NT; base < n; base += (uint64_t)gridDim.x * NT) {
        // the wave's 64 keys lie in the local bins [lb0, lb1] (wave-uniform searches); a lane searches there
        const uint64_t w0 = base + (uint64_t)wid * 64;
        if (w0 >= n) continue;
        const uint64_t w1 = w0 + 63 < n ? w0 + 63 : n - 1;
        const uint32_t lb0 = store_bin_of(bin_off, 0, t.nlb - 1, w0);
        const uint32_t lb1 = store_bin_of(bin_off, lb0, t.nlb - 1, w1);
        const uint64_t i = w0 + lane;
        if (i >= n) continue;
        const KmerKey f = query_load_key<KW>(keys, i);
        const uint32_t cnt = counts[i];
        if constexpr (KW == 2)
            sum += store_term(f.hi, 2 * i) + store_term(f.lo, 2 * i + 1);
        else
            sum += store_term(f.lo, i);
        sum += store_term(cnt, (1ull << 63) + i);
        kmers += cnt;
        const uint32_t lb = store_bin_of(bin_off, lb0, lb1, i);
        uint32_t why = 0;
        if (!key_is_kmer(f, t.k)) {
            why = STORE_BAD_BITS;
        } else {
            const KmerKey r = revcomp_key<KW == 2>(f, t.k);
            const uint32_t b = bin_of_signature(kmer_signature<KW == 2>(f, r, t.k, t.m), t.fm);
            bool here;
            if (t.owner)
                here = t.owner[b] == t.rank && t.local[b] == lb;
            else
                here = b == t.rank + lb * t.G;
            if (key_less(r, f)) {
                why = STORE_BAD_STRAND;
            } else if (!here) {
                why = STORE_BAD_BIN;
            } else if (i > bin_off[lb]) {
                const KmerKey p = query_load_key<KW>(keys, i - 1);
                if (p.hi == f.hi && p.lo == f.lo)
                    why = STORE_BAD_DUP;
                else if (!key_less(p, f))
                    why = STORE_BAD_ORDER;
            }
            if (!why && cnt == 0) why = STORE_BAD_COUNT;
        }
        if (why) {
            const uint64_t code = ~((i << 3) | why);
            bad = code > bad ? code : bad;
        }
    }
    // wave first, as the FASTQ stage reports its first malformed record: one atomic per wave that saw one
    bad = wave_incl_max<uint64_t>(bad);
    if (lane == 63 && bad) atomicMax(&res[0], (unsigned long long)bad);
    sum = wave_incl_sum<uint64_t>(sum);
    kmers = wave_incl_sum<uint64_t>(kmers);
    if (lane == 63) s_sum[0][wid] = sum, s_sum[1][wid] = kmers;
    __syncthreads();
    if (threadIdx.x < 2) {
        uint64_t v = 0;
#pragma unroll
        for (int w = 0; w < NT / 64; ++w) v += s_sum[threadIdx.x][w];
        if (v) atomicAdd(&res[1 + threadIdx.x], (unsigned long long)v);
    }
}

hipError_t launch_store_verify(int KW, const StoreTables &t, const uint64_t *keys, const uint32_t *counts, uint64_t n,
                               const uint64_t *bin_off, unsigned long long *res, hipStream_t s) {
    if (!n || !t.nlb) return hipSuccess;
    const unsigned grid = (unsigned)std::min<uint64_t>((n + NT - 1) / NT, STORE_GRID_MAX);
    if (KW == 1)
        k_store_verify<1><<<grid, NT, 0, s>>>(t, keys, counts, n, bin_off, res);
    else
        k_store_verify<2><<<grid, NT, 0, s>>>(t, keys, counts, n, bin_off, res);
    return hipGetLastError();
}

// the checksum alone, over arrays already known good (fk_save): res[1] += terms, res[2] += counts
__global__ __launch_bounds__(NT) void k_store_checksum(const uint64_t *__restrict__ words, uint64_t nwords,
                                                       const uint32_t *__restrict__ counts, uint64_t n,
                                                       unsigned long long *__restrict__ res) {
    __shared__ uint64_t s_sum[2][NT / 64];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const uint64_t stride = (uint64_t)gridDim.x * NT;
    uint64_t sum = 0, kmers = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x; i < nwords; i += stride) sum += store_term(words[i], i);
    for (uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x; i < n; i += stride) {
        const uint32_t c = counts[i];
        sum += store_term(c, (1ull << 63) + i);
        kmers += c;
    }
    sum = wave_incl_sum<uint64_t>(sum);
    kmers = wave_incl_sum<uint64_t>(kmers);
    if (lane == 63) s_sum[0][wid] = sum, s_sum[1][wid] = kmers;
    __syncthreads();
    if (threadIdx.x < 2) {
        uint64_t v = 0;
#pragma unroll
        for (int w = 0; w < NT / 64; ++w) v += s_sum[threadIdx.x][w];
        if (v) atomicAdd(&res[1 + threadIdx.x], (unsigned long long)v);
    }
}

hipError_t launch_store_checksum(const uint64_t *words, uint64_t nwords, const uint32_t *counts, uint64_t n,
                                 unsigned long long *res, hipStream_t s) {
    if (!nwords && !n) return hipSuccess;
    const unsigned grid = (unsigned)std::min<uint64_t>((std::max(nwords, n) + NT - 1) / NT, STORE_GRID_MAX);
    k_store_checksum<<<grid, NT, 0, s>>>(words, nwords, counts, n, res);
    return hipGetLastError();
}

// cell_base[g], g = (lb << F) + cell: the dense index of the first key of local bin lb whose cell (top
// F bits) is >= cell -- the bin's keys ascend, so their cells do; cell_base[nlb << F] = the keys
template <int KW>
__global__ __launch_bounds__(NT) void k_store_cells(const uint64_t *__restrict__ keys,
                                                    const uint64_t *__restrict__ bin_off, uint32_t nlb, int k, int F,
                                                    uint64_t *__restrict__ cell_base) {
    const uint64_t g = (uint64_t)blockIdx.x * NT + threadIdx.x, ncell_all = (uint64_t)nlb << F;
    if (g > ncell_all) return;
    if (g == ncell_all) {
        cell_base[g] = bin_off[nlb];
        return;
    }
    const uint32_t lb = (uint32_t)(g >> F), cell = (uint32_t)(g & ((1u << F) - 1u));
    uint64_t lo = bin_off[lb], hi = bin_off[lb + 1];
    if (cell == 0) hi = lo;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (key_cell(query_load_key<KW>(keys, mid), k, F) < cell)
            lo = mid + 1;
        else
            hi = mid;
    }
    cell_base[g] = lo;
}

// cell_total[g] = the cell's keys; res[3] |= 1 for a cell of 2^32 keys or more (a Bucket's n is 32 bits)
__global__ __launch_bounds__(NT) void k_store_cell_totals(const uint64_t *__restrict__ cell_base, uint64_t ncell_all,
                                                          uint64_t *__restrict__ cell_total,
                                                          unsigned long long *__restrict__ res) {
    const uint64_t g = (uint64_t)blockIdx.x * NT + threadIdx.x;
    if (g >= ncell_all) return;
    const uint64_t t = cell_base[g + 1] - cell_base[g];
    cell_total[g] = t;
    if (t >> 32) atomicOr(&res[3], 1ull);
}

hipError_t launch_store_cells(int KW, const uint64_t *keys, const uint64_t *bin_off, uint32_t nlb, int k, int F,
                              uint64_t *cell_base, uint64_t *cell_total, unsigned long long *res, hipStream_t s) {
    const uint64_t ncell_all = (uint64_t)nlb << F;
    if (!nlb) return hipSuccess;
    const unsigned grid = (unsigned)((ncell_all + 1 + NT - 1) / NT);
    if (KW == 1)
        k_store_cells<1><<<grid, NT, 0, s>>>(keys, bin_off, nlb, k, F, cell_base);
    else
        k_store_cells<2><<<grid, NT, 0, s>>>(keys, bin_off, nlb, k, F, cell_base);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    k_store_cell_totals<<<(unsigned)((ncell_all + NT - 1) / NT), NT, 0, s>>>(cell_base, ncell_all, cell_total, res);
    return hipGetLastError();
}

// k_bucket_finish for a result without gaps, the number of buckets read on the device (*nb_dev, at most
// nb_max): bucket i ends where bucket i + 1 begins, the last one at *total_keys; dense_off[i] = begin
__global__ __launch_bounds__(NT) void k_store_finish(Bucket *__restrict__ buckets, const uint64_t *__restrict__ nb_dev,
                                                     uint64_t nb_max, uint32_t nlb, int F,
                                                     const uint64_t *__restrict__ total_keys,
                                                     uint64_t *__restrict__ dense_off) {
    const uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x, nb = *nb_dev < nb_max ? *nb_dev : nb_max;
    if (i == 0 && nb == 0) dense_off[0] = 0;
    if (i >= nb) return;
    const uint32_t ncell = 1u << F;
    const Bucket b = buckets[i];
    uint64_t e_beg = *total_keys, g1 = (uint64_t)nlb << F;
    if (i + 1 < nb) {
        const Bucket nx = buckets[i + 1];
        e_beg = nx.begin;
        g1 = ((uint64_t)nx.lbin << F) + nx.c0;
    } else {
        dense_off[nb] = e_beg;
    }
    buckets[i].n = (uint32_t)(e_beg - b.begin);
    buckets[i].c1 = (g1 >> F) == b.lbin ? (uint32_t)(g1 & (ncell - 1)) : ncell;
    dense_off[i] = b.begin;
}

hipError_t launch_store_finish(Bucket *buckets, const uint64_t *nb_dev, uint64_t nb_max, uint32_t nlb, int F,
                               const uint64_t *total_keys, uint64_t *dense_off, hipStream_t s) {
    const unsigned grid = (unsigned)((std::max<uint64_t>(nb_max, 1) + NT - 1) / NT);
    k_store_finish<<<grid, NT, 0, s>>>(buckets, nb_dev, nb_max, nlb, F, total_keys, dense_off);
    return hipGetLastError();
}
