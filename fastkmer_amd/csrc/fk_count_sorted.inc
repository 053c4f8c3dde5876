// fk_count_sorted.inc -- included by fk_kernels.hip inside namespace fk.
// Stages 4-5 of the sorted count (useHT=0): expansion of super-k-mer records
// into canonical k-mers, bucketing by (bin, cell) and the exact count of each
// bucket in LDS.  Together they produce, per bin, the ascending
// (k-mer, count) list of extractKXmers (SparkBinKmerCounter.scala:428-660).

// ---------------------------------------------------------------------------
// 4b. expand (the run loop of extractKXmers, SBKC:484-524), two passes over
//     each chunk's records.  k_expand_hist: LDS histogram of the chunk's
//     canonical k-mers by cell = top F bits -> hist[chunk][cell].
//     k_cell_prefix turns the histograms into per-(chunk, cell) write offsets
//     inside the bin-major (bin, cell) layout; k_expand_scatter recomputes the
//     k-mers and writes each one to its (bin, cell) run, so every bucket of
//     consecutive cells is one contiguous range of keys[].
// ---------------------------------------------------------------------------

// Flattened expansion: a wave loads 64 records (one per lane), stages their
// bases in LDS and maps each of the wave's k-mer slots t < sum(n) to its
// record, so every lane handles one k-mer per iteration whatever the record
// lengths (1..16 k-mers) -- a thread-per-record loop leaves ~2/3 of the lanes
// idle.  fn(key) is called once per k-mer of the chunk.
struct ExpandLds {
    uint64_t s0[NT], s1[NT], s2[NT];
    uint32_t first[NT];  // first k-mer slot of each lane's record (wave-local)
    uint8_t owner[NT / 64][64 * SIG_PPT];
};

template <int W, int KW, typename Fn>
__device__ __forceinline__ void for_each_chunk_kmer(const uint64_t *__restrict__ rec, const Chunk &ch, int k,
                                                    ExpandLds &e, Fn fn) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const uint64_t nrec = ch.rec_end - ch.rec_begin;
    const uint64_t rounds = (nrec + NT - 1) / NT;
    for (uint64_t rd = 0; rd < rounds; ++rd) {
        const uint64_t i = ch.rec_begin + rd * NT + threadIdx.x;
        uint32_t n = 0;
        if (i < ch.rec_end) {
            RecView<W> r;
            r.load(rec, i);
            n = r.n;
            e.s0[threadIdx.x] = r.s0;
            e.s1[threadIdx.x] = r.s1;
            if (W == 3) e.s2[threadIdx.x] = r.s2;
        }
        const uint32_t inc = wave_incl_sum<uint32_t>(n);
        const uint32_t total = __shfl(inc, 63, 64);
        const uint32_t first = inc - n;
        e.first[threadIdx.x] = first;
        for (uint32_t q = 0; q < n; ++q) e.owner[wid][first + q] = (uint8_t)lane;
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        for (uint32_t t = lane; t < total; t += 64) {
            const uint32_t o = e.owner[wid][t];
            const uint32_t slot = (wid << 6) + o;
            RecView<W> r;
            r.s0 = e.s0[slot];
            r.s1 = e.s1[slot];
            r.s2 = (W == 3) ? e.s2[slot] : 0;
            fn(kmer_canon<W, KW>(r, (int)(t - e.first[slot]), k));
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    }
}

template <int W, int KW>
__global__ __launch_bounds__(NT) void k_expand_hist(const uint64_t *__restrict__ rec, const Chunk *__restrict__ chunks,
                                                    int k, int F, uint32_t *__restrict__ hist) {
    extern __shared__ uint32_t s_h[];
    __shared__ ExpandLds e;
    const uint32_t ncell = 1u << F;
    for (uint32_t c = threadIdx.x; c < ncell; c += NT) s_h[c] = 0;
    __syncthreads();
    const Chunk ch = chunks[blockIdx.x];
    for_each_chunk_kmer<W, KW>(rec, ch, k, e, [&](typename KeyOf<KW>::T key) {
        atomicAdd(&s_h[cell_of(key, k, F)], 1u);
    });
    __syncthreads();
    uint32_t *row = hist + (uint64_t)blockIdx.x * ncell;
    for (uint32_t c = threadIdx.x; c < ncell; c += NT) row[c] = s_h[c];
}

// thread per (local bin, cell): exclusive prefix over the bin's chunks (in
// place) and the cell total
__global__ void k_cell_prefix(const uint32_t *bin_chunk_begin, uint32_t nlbins, int F, uint32_t *hist,
                              uint64_t *cell_total) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t ncell = 1u << F;
    if (g >= (uint64_t)nlbins * ncell) return;
    const uint32_t lb = (uint32_t)(g >> F), c = (uint32_t)(g & (ncell - 1));
    uint32_t acc = 0;
    for (uint32_t ch = bin_chunk_begin[lb]; ch < bin_chunk_begin[lb + 1]; ++ch) {
        uint32_t *p = hist + (uint64_t)ch * ncell + c;
        const uint32_t v = *p;
        *p = acc;
        acc += v;
    }
    cell_total[g] = acc;
}

template <int W, int KW>
__global__ __launch_bounds__(NT) void k_expand_scatter(const uint64_t *__restrict__ rec,
                                                       const Chunk *__restrict__ chunks, int k, int F,
                                                       const uint32_t *__restrict__ hist,
                                                       const uint64_t *__restrict__ cell_base,
                                                       uint64_t *__restrict__ keys) {
    extern __shared__ unsigned long long s_cur[];
    __shared__ ExpandLds e;
    const uint32_t ncell = 1u << F;
    const Chunk ch = chunks[blockIdx.x];
    const uint32_t *pre = hist + (uint64_t)blockIdx.x * ncell;
    const uint64_t *base = cell_base + ((uint64_t)ch.lbin << F);
    for (uint32_t c = threadIdx.x; c < ncell; c += NT) s_cur[c] = base[c] + pre[c];
    __syncthreads();
    for_each_chunk_kmer<W, KW>(rec, ch, k, e, [&](typename KeyOf<KW>::T key) {
        const uint64_t pos = atomicAdd(&s_cur[cell_of(key, k, F)], 1ull);
        store_key(keys, pos, key);
    });
}

// ---- rolling expansion ----------------------------------------------------
// A thread expands its own record: the first k-mer and its reverse complement
// are built once, then every further base is one shift on each strand (the
// flattened loop above rebuilds both strands per k-mer).

__device__ __forceinline__ void record_keys64(const RecView<2> &r, int k, uint64_t (&key)[16]) {
    const uint64_t mask = k == 32 ? ~0ull : ((1ull << (2 * k)) - 1ull);
    uint64_t fwd = k == 32 ? r.s0 : r.s0 >> (64 - 2 * k);
    uint64_t yh = k == 32 ? r.s1 : (r.s0 << (2 * k)) | (r.s1 >> (64 - 2 * k));  // bases k.. at the top
    uint64_t yl = k == 32 ? 0 : r.s1 << (2 * k);
    uint64_t rc = revcomp64(fwd, k);
    const int top = 2 * k - 2;
    key[0] = fwd < rc ? fwd : rc;
#pragma unroll
    for (int j = 1; j < 16; ++j) {
        const uint64_t b = yh >> 62;
        yh = (yh << 2) | (yl >> 62);
        yl <<= 2;
        fwd = ((fwd << 2) | b) & mask;
        rc = (rc >> 2) | ((b ^ 3ull) << top);
        key[j] = fwd < rc ? fwd : rc;
    }
}

// k in 33..63 (W = 3): the same rolling expansion on 128-bit keys
__device__ __forceinline__ void record_keys128(const RecView<3> &r, int k, u128 (&key)[16]) {
    const u128 mask = ((u128)1 << (2 * k)) - 1;
    const u128 x = ((u128)r.s0 << 64) | r.s1;  // bases 0..63
    u128 fwd = x >> (128 - 2 * k);
    u128 rest = (x << (2 * k)) | ((u128)r.s2 << (2 * k - 64));  // bases k.. at the top (2k in 66..126)
    u128 rc = revcomp128(fwd, k);
    const int top = 2 * k - 2;
    key[0] = fwd < rc ? fwd : rc;
#pragma unroll
    for (int j = 1; j < 16; ++j) {
        const uint32_t b = (uint32_t)(rest >> 126);
        rest <<= 2;
        fwd = ((fwd << 2) | b) & mask;
        rc = (rc >> 2) | ((u128)(b ^ 3u) << top);
        key[j] = fwd < rc ? fwd : rc;
    }
}

template <int KW>
struct RollKeys;
template <>
struct RollKeys<1> {
    static constexpr int W = 2;
    __device__ static void get(const RecView<2> &r, int k, uint64_t (&key)[16]) { record_keys64(r, k, key); }
};
template <>
struct RollKeys<2> {
    static constexpr int W = 3;
    __device__ static void get(const RecView<3> &r, int k, u128 (&key)[16]) { record_keys128(r, k, key); }
};

// Bin-resident cell totals: one workgroup per local bin walks
// the bin's chunks in order with the bin's cell histogram resident in LDS, so
// the cell totals are plain stores once per bin (no global atomics, which at
// F = 15 cost 32K per chunk), and each chunk's super-cell counts come out as
// the exclusive prefix over the bin's earlier chunks (k_cell_prefix is not
// needed).  Super-cell sums read the histogram with a per-thread rotation so
// the 2^F2-strided reads spread over the LDS banks.
constexpr int BH_NT = 1024;

template <int KW>
__global__ __launch_bounds__(BH_NT) void k_expand_hist_bin(const uint64_t *__restrict__ rec,
                                                           const Chunk *__restrict__ chunks,
                                                           const uint32_t *__restrict__ bin_chunk_begin, int k,
                                                           int F, int F2,
                                                           unsigned long long *__restrict__ cell_total,
                                                           uint32_t *__restrict__ hist_sc) {
    typedef typename KeyOf<KW>::T K;
    constexpr int W = RollKeys<KW>::W;
    extern __shared__ uint32_t s_h[];  // [2^F] cell counts, then [2^(F-F2)] running super-cell sums
    const uint32_t ncell = 1u << F, S = ncell >> F2, m2 = (1u << F2) - 1;
    uint32_t *s_run = s_h + ncell;
    for (uint32_t c = threadIdx.x; c < ncell; c += BH_NT) s_h[c] = 0;
    for (uint32_t d = threadIdx.x; d < S; d += BH_NT) s_run[d] = 0;
    __syncthreads();
    const uint32_t lb = blockIdx.x;
    const int cs = 2 * k - F;
    const uint32_t c0 = bin_chunk_begin[lb], c1 = bin_chunk_begin[lb + 1];
    for (uint32_t ci = c0; ci < c1; ++ci) {
        const Chunk ch = chunks[ci];
        for (uint64_t i = ch.rec_begin + threadIdx.x; i < ch.rec_end; i += BH_NT) {
            RecView<W> r;
            r.load(rec, i);
            K key[16];
            RollKeys<KW>::get(r, k, key);
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (j < (int)r.n) atomicAdd(&s_h[(uint32_t)(key[j] >> cs)], 1u);
        }
        __syncthreads();
        uint32_t *row = hist_sc + (uint64_t)ci * S;
        for (uint32_t d = threadIdx.x; d < S; d += BH_NT) {
            uint32_t acc = 0;
            for (uint32_t j = 0; j <= m2; ++j) acc += s_h[(d << F2) + ((j + d) & m2)];
            row[d] = s_run[d];
            s_run[d] = acc;  // cumulative over chunks c0..ci (s_h is never cleared)
        }
        __syncthreads();
    }
    unsigned long long *tot = cell_total + ((uint64_t)lb << F);
    for (uint32_t c = threadIdx.x; c < ncell; c += BH_NT) tot[c] = s_h[c];
}

// The same over pieces of bins: piece blockIdx covers chunks [cb, ce) of local bin lb (a bin with
// many chunks is split so that the workgroups balance over the CUs: at F = 15 a workgroup holds
// 130 KB of LDS, one per CU, and one workgroup per bin waits for the largest bin).  A piece writes
// its chunks' super-cell counts as the exclusive prefix inside the piece and its per-super-cell
// totals to piece_tot; k_hist_piece_fix adds the earlier pieces' totals.  Cell totals: plain stores
// when the piece is the whole bin, else atomic adds into the zeroed cell_total.
template <int KW>
__global__ __launch_bounds__(BH_NT) void k_expand_hist_piece(const uint64_t *__restrict__ rec,
                                                             const Chunk *__restrict__ chunks,
                                                             const uint4 *__restrict__ pieces, int k, int F, int F2,
                                                             unsigned long long *__restrict__ cell_total,
                                                             uint32_t *__restrict__ hist_sc,
                                                             uint32_t *__restrict__ piece_tot) {
    typedef typename KeyOf<KW>::T K;
    constexpr int W = RollKeys<KW>::W;
    extern __shared__ uint32_t s_h[];
    const uint32_t ncell = 1u << F, S = ncell >> F2, m2 = (1u << F2) - 1;
    uint32_t *s_run = s_h + ncell;
    for (uint32_t c = threadIdx.x; c < ncell; c += BH_NT) s_h[c] = 0;
    for (uint32_t d = threadIdx.x; d < S; d += BH_NT) s_run[d] = 0;
    __syncthreads();
    const uint4 pc = pieces[blockIdx.x];  // lb, chunk begin, chunk end, whole-bin flag
    const int cs = 2 * k - F;
    for (uint32_t ci = pc.y; ci < pc.z; ++ci) {
        const Chunk ch = chunks[ci];
        for (uint64_t i = ch.rec_begin + threadIdx.x; i < ch.rec_end; i += BH_NT) {
            RecView<W> r;
            r.load(rec, i);
            K key[16];
            RollKeys<KW>::get(r, k, key);
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (j < (int)r.n) atomicAdd(&s_h[(uint32_t)(key[j] >> cs)], 1u);
        }
        __syncthreads();
        uint32_t *row = hist_sc + (uint64_t)ci * S;
        for (uint32_t d = threadIdx.x; d < S; d += BH_NT) {
            uint32_t acc = 0;
            for (uint32_t j = 0; j <= m2; ++j) acc += s_h[(d << F2) + ((j + d) & m2)];
            row[d] = s_run[d];
            s_run[d] = acc;
        }
        __syncthreads();
    }
    for (uint32_t d = threadIdx.x; d < S; d += BH_NT) piece_tot[(uint64_t)blockIdx.x * S + d] = s_run[d];
    unsigned long long *tot = cell_total + ((uint64_t)pc.x << F);
    if (pc.w) {
        for (uint32_t c = threadIdx.x; c < ncell; c += BH_NT) tot[c] = s_h[c];
    } else {
        for (uint32_t c = threadIdx.x; c < ncell; c += BH_NT)
            if (s_h[c]) atomicAdd(&tot[c], (unsigned long long)s_h[c]);
    }
}

// pieces after a bin's first: every chunk's super-cell prefix += the earlier pieces' totals
__global__ __launch_bounds__(NT) void k_hist_piece_fix(const uint4 *__restrict__ pieces, const uint32_t *first_piece,
                                                       int S, const uint32_t *__restrict__ piece_tot,
                                                       uint32_t *__restrict__ hist_sc) {
    const uint4 pc = pieces[blockIdx.x];
    const uint32_t f = first_piece[blockIdx.x];
    if (f == blockIdx.x) return;
    for (uint32_t d = threadIdx.x; d < (uint32_t)S; d += NT) {
        uint32_t add = 0;
        for (uint32_t q = f; q < blockIdx.x; ++q) add += piece_tot[(uint64_t)q * S + d];
        for (uint32_t ci = pc.y; ci < pc.z; ++ci) hist_sc[(uint64_t)ci * S + d] += add;
    }
}

// The one-level expansion (k = 64 only: W = 3, 128-bit keys; k <= 63 takes the two-level one,
// fk_expand2.inc)
hipError_t launch_expand_hist(int W, const uint64_t *rec, const Chunk *chunks, uint32_t nchunks, int k, int F,
                              uint32_t *hist, hipStream_t s) {
    if (!nchunks) return hipSuccess;
    if (W != 3) return hipErrorInvalidValue;
    const size_t lds = (size_t)4 << F;  // F <= MAX_FINE_BITS = 15: up to 128 KB
    hipError_t e = part_lds_attr((const void *)k_expand_hist<3, 2>, lds);
    if (e != hipSuccess) return e;
    k_expand_hist<3, 2><<<nchunks, NT, lds, s>>>(rec, chunks, k, F, hist);
    return hipGetLastError();
}

hipError_t launch_expand_hist_bin(int KW, const uint64_t *rec, const Chunk *chunks, const uint32_t *bin_chunk_begin,
                                  uint32_t nlbins, int k, int F, int F2, uint64_t *cell_total, uint32_t *hist_sc,
                                  hipStream_t s) {
    if (!nlbins) return hipSuccess;
    const size_t lds = ((size_t)4 << F) + ((size_t)4 << (F - F2));  // F <= 15: <= 130 KB
    const void *fn = KW == 1 ? (const void *)k_expand_hist_bin<1> : (const void *)k_expand_hist_bin<2>;
    hipError_t e = part_lds_attr(fn, lds);
    if (e != hipSuccess) return e;
    if (KW == 1)
        k_expand_hist_bin<1><<<nlbins, BH_NT, lds, s>>>(rec, chunks, bin_chunk_begin, k, F, F2,
                                                        (unsigned long long *)cell_total, hist_sc);
    else
        k_expand_hist_bin<2><<<nlbins, BH_NT, lds, s>>>(rec, chunks, bin_chunk_begin, k, F, F2,
                                                        (unsigned long long *)cell_total, hist_sc);
    return hipGetLastError();
}

hipError_t launch_expand_hist_pieces(int KW, const uint64_t *rec, const Chunk *chunks, const uint4 *pieces,
                                     const uint32_t *first_piece, uint32_t npieces, int k, int F, int F2,
                                     uint64_t *cell_total, uint32_t *hist_sc, uint32_t *piece_tot, hipStream_t s) {
    if (!npieces) return hipSuccess;
    const size_t lds = ((size_t)4 << F) + ((size_t)4 << (F - F2));
    const void *fn = KW == 1 ? (const void *)k_expand_hist_piece<1> : (const void *)k_expand_hist_piece<2>;
    hipError_t e = part_lds_attr(fn, lds);
    if (e != hipSuccess) return e;
    if (KW == 1)
        k_expand_hist_piece<1><<<npieces, BH_NT, lds, s>>>(rec, chunks, pieces, k, F, F2,
                                                           (unsigned long long *)cell_total, hist_sc, piece_tot);
    else
        k_expand_hist_piece<2><<<npieces, BH_NT, lds, s>>>(rec, chunks, pieces, k, F, F2,
                                                           (unsigned long long *)cell_total, hist_sc, piece_tot);
    k_hist_piece_fix<<<npieces, NT, 0, s>>>(pieces, first_piece, 1 << (F - F2), piece_tot, hist_sc);
    return hipGetLastError();
}

hipError_t launch_cell_prefix(const uint32_t *bin_chunk_begin, uint32_t nlbins, int F, uint32_t *hist,
                              uint64_t *cell_total, hipStream_t s) {
    const uint64_t n = (uint64_t)nlbins << F;
    if (!n) return hipSuccess;
    k_cell_prefix<<<(unsigned)((n + NT - 1) / NT), NT, 0, s>>>(bin_chunk_begin, nlbins, F, hist, cell_total);
    return hipGetLastError();
}

hipError_t launch_expand_scatter(int W, const uint64_t *rec, const Chunk *chunks, uint32_t nchunks, int k, int F,
                                 const uint32_t *hist, const uint64_t *cell_base, uint64_t *keys, hipStream_t s) {
    if (!nchunks) return hipSuccess;
    if (W != 3) return hipErrorInvalidValue;
    const size_t lds = (size_t)8 << F;  // the caller caps F at 14 for this path: <= 128 KB
    hipError_t e = part_lds_attr((const void *)k_expand_scatter<3, 2>, lds);
    if (e != hipSuccess) return e;
    k_expand_scatter<3, 2><<<nchunks, NT, lds, s>>>(rec, chunks, k, F, hist, cell_base, keys);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// 4c. buckets: runs of consecutive cells of one bin.  A bucket starts at
//     cell 0 of every bin, at every cell larger than small_cap, after such a
//     cell, and where the in-bin prefix crosses a multiple of `group`; with
//     small_cap + group <= the LDS capacity a bucket of small cells always
//     fits.  Single cells above the capacity take the large-bucket path.
// ---------------------------------------------------------------------------

__global__ void k_bucket_flags(const uint64_t *cell_base, const uint64_t *cell_total, uint32_t nlbins, int F,
                               uint32_t small_cap, uint32_t group, uint32_t *flags) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t ncell = 1u << F;
    if (g >= (uint64_t)nlbins * ncell) return;
    const uint32_t c = (uint32_t)(g & (ncell - 1));
    uint32_t f = 1;
    if (c != 0) {
        const uint64_t b0 = cell_base[g - c];
        const uint64_t p = cell_base[g] - b0;
        const uint64_t t = cell_total[g];
        const uint64_t tp = cell_total[g - 1];
        const uint64_t pp = p - tp;
        f = (t > small_cap) || (tp > small_cap) || (p / group != pp / group);
    }
    flags[g] = f;
}

__global__ void k_bucket_write(const uint64_t *cell_base, const uint32_t *flags, const uint64_t *flag_scan,
                               uint32_t nlbins, int F, Bucket *buckets) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= ((uint64_t)nlbins << F)) return;
    if (!flags[g]) return;
    Bucket b;
    b.begin = cell_base[g];
    b.n = 0;
    b.lbin = (uint32_t)(g >> F);
    b.c0 = (uint32_t)(g & ((1u << F) - 1));
    b.c1 = 0;
    buckets[flag_scan[g]] = b;
}

hipError_t launch_bucket_flags(const uint64_t *cell_base, const uint64_t *cell_total, uint32_t nlbins, int F,
                               uint32_t small_cap, uint32_t group, uint32_t *flags, hipStream_t s) {
    const uint64_t n = (uint64_t)nlbins << F;
    if (!n) return hipSuccess;
    k_bucket_flags<<<(unsigned)((n + NT - 1) / NT), NT, 0, s>>>(cell_base, cell_total, nlbins, F, small_cap, group,
                                                               flags);
    return hipGetLastError();
}

hipError_t launch_bucket_write(const uint64_t *cell_base, const uint32_t *flags, const uint64_t *flag_scan,
                               uint32_t nlbins, int F, uint64_t nbuckets, uint64_t total_keys, Bucket *buckets,
                               hipStream_t s) {
    const uint64_t n = (uint64_t)nlbins << F;
    if (!n) return hipSuccess;
    k_bucket_write<<<(unsigned)((n + NT - 1) / NT), NT, 0, s>>>(cell_base, flags, flag_scan, nlbins, F, buckets);
    return hipGetLastError();
}

// (BucketSrc, fk_internal.h: a bucket's keys in one array or in the staged pieces' arrays)
// where key i of a bucket lives: b[0] + i below p[1], b[1] + i below p[2], ... (the unused pieces
// have p = ~0u); indexed with constants only (unrolled), so the view stays in registers
struct BucketView {
    const uint64_t *b[STAGE_MAXP];
    uint32_t p[STAGE_MAXP];  // p[0] unused
};

template <int KW = 1>
__device__ __forceinline__ BucketView bucket_view(const BucketSrc &src, const Bucket &b) {
    BucketView v;
    constexpr int NPC = stage_npc<KW>();
    if (src.np == 0) {
#pragma unroll
        for (int q = 0; q < NPC; ++q) v.b[q] = src.keys + KW * b.begin, v.p[q] = ~0u;
        return v;
    }
    const uint64_t g0 = ((uint64_t)b.lbin << src.F) + b.c0, g1 = ((uint64_t)b.lbin << src.F) + b.c1;
    // piece q's range of the bucket: [pcb[q][g0], pcb[q][g1]); base so that key i is base + i
    uint32_t acc = 0;
#pragma unroll
    for (int q = 0; q < NPC; ++q) {
        if (q == 0 || q < src.np) {
            const uint64_t s0 = src.pcb[q][g0], s1 = src.pcb[q][g1];
            v.b[q] = src.pk[q] + KW * ((int64_t)s0 - (int64_t)acc);
            v.p[q] = q ? acc : 0u;
            acc += (uint32_t)(s1 - s0);
        } else {
            v.b[q] = v.b[q - 1];
            v.p[q] = ~0u;
        }
    }
    return v;
}

// the view from a bucket's precomputed piece starts (one load instead of 2 np dependent ones)
template <int KW = 1>
__device__ __forceinline__ BucketView bucket_view_starts(const BucketSrc &src, const PieceStarts &ps) {
    BucketView v;
    v.b[0] = src.pk[0] + KW * ps.s[0];
    v.p[0] = 0;
#pragma unroll
    for (int q = 1; q < stage_npc<KW>(); ++q) {
        v.b[q] = src.pk[q] + KW * ((int64_t)ps.s[q] - (int64_t)ps.pre[q]);
        v.p[q] = ps.pre[q];
    }
    return v;
}

// Each bucket's size and end cell from the next bucket's start (k_bucket_write leaves n = c1 = 0)
// and, with staged pieces, its piece starts.  The last bucket ends at *total_keys, the last word of
// the cell offsets' scan (folded pieces hold fewer keys than the job has k-mers: the host's count
// would not do).  One bucket per thread; bucket i ends where i + 1
// starts (every bin's first bucket starts at its cell 0), so a piece's cell offset at the end comes
// from the next lane's read (the wave's last lane reads its own).
template <bool PIECES>
__global__ __launch_bounds__(NT) void k_bucket_finish(BucketSrc src, Bucket *__restrict__ buckets, uint64_t nb,
                                                      uint32_t nlbins, const uint64_t *__restrict__ total_keys,
                                                      PieceStarts *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x;
    const bool mine = i < nb;  // every lane takes part in the shuffles below
    const uint32_t ncell = 1u << src.F;
    Bucket b{};
    uint64_t e_beg = *total_keys, g1 = (uint64_t)nlbins << src.F;
    if (mine) {
        b = buckets[i];
        if (i + 1 < nb) {
            const Bucket nx = buckets[i + 1];
            e_beg = nx.begin;
            g1 = ((uint64_t)nx.lbin << src.F) + nx.c0;
        }
        buckets[i].n = (uint32_t)(e_beg - b.begin);
        buckets[i].c1 = (g1 >> src.F) == b.lbin ? (uint32_t)(g1 & (ncell - 1)) : ncell;
    }
    if constexpr (PIECES) {
        const uint64_t g0 = ((uint64_t)b.lbin << src.F) + b.c0;
        const bool own_end = (threadIdx.x & 63) == 63 || i + 1 >= nb;
        PieceStarts ps;
        uint32_t acc = 0;
#pragma unroll
        for (int p = 0; p < STAGE_MAXP; ++p) {
            if (p < src.np) {  // uniform
                const uint64_t s0 = mine ? src.pcb[p][g0] : 0;
                uint64_t s1 = (uint64_t)__shfl_down((long long)s0, 1, 64);
                if (mine && own_end) s1 = src.pcb[p][g1];
                ps.s[p] = s0;
                ps.pre[p] = acc;
                acc += (uint32_t)(s1 - s0);
            } else {
                ps.s[p] = 0;
                ps.pre[p] = ~0u;
            }
        }
        if (mine) out[i] = ps;
    }
}

hipError_t launch_bucket_finish(const BucketSrc &src, Bucket *buckets, uint64_t nb, uint32_t nlbins,
                                const uint64_t *total_keys, PieceStarts *out, hipStream_t s) {
    if (!nb) return hipSuccess;
    const unsigned grid = (unsigned)((nb + NT - 1) / NT);
    if (src.np > 0)
        k_bucket_finish<true><<<grid, NT, 0, s>>>(src, buckets, nb, nlbins, total_keys, out);
    else
        k_bucket_finish<false><<<grid, NT, 0, s>>>(src, buckets, nb, nlbins, total_keys, out);
    return hipGetLastError();
}


// a streaming load from global memory: the pointers built by bucket_key_ptr (integer arithmetic)
// would be generic, and a generic (flat) load also counts in the LDS wait counter, so every LDS wait
// of a wave tier would wait for the keys it prefetched
template <class T>
__device__ __forceinline__ T ldg_nt(const void *p) {
    typedef const __attribute__((address_space(1))) T *gp;
    return __builtin_nontemporal_load((gp)(uintptr_t)p);
}


template <int KW = 1>
__device__ __forceinline__ const uint64_t *bucket_key_ptr(const BucketView &v, uint32_t i) {
    // p[1] <= p[2] <= ...: add the steps between consecutive bases (a chain of pointer selects is
    // turned into a lookup table in scratch memory by the compiler)
    uintptr_t a = (uintptr_t)v.b[0] + (uintptr_t)i * (8u * KW);
#pragma unroll
    for (int q = 1; q < stage_npc<KW>(); ++q) a += i >= v.p[q] ? (uintptr_t)v.b[q] - (uintptr_t)v.b[q - 1] : 0;
    return reinterpret_cast<const uint64_t *>(a);
}

// A bucket's rows of 64 keys, 64 rows at a time: lane r works out row r's piece base once (the
// compares run on the lanes together, not per row on the scalar unit: ~25 scalar instructions per row
// before) and whether a piece boundary falls inside the row; a row then takes its base with two lane
// reads, a row across a boundary bucket_key_ptr's per-lane selects.
struct RowBases {
    uintptr_t base;  // lane r: row r's piece base (key i of the row at base + KW * 8 * i)
    uint64_t inner;  // bit r: a piece boundary inside row r
};
template <int KW = 1>
__device__ __forceinline__ RowBases row_bases(const BucketView &v, uint32_t first_row = 0) {
    // lane r: row first_row + r
    const uint32_t r0 = (first_row + (threadIdx.x & 63)) * 64u;
    uintptr_t a = (uintptr_t)v.b[0];
    bool inner = false;
#pragma unroll
    for (int q = 1; q < stage_npc<KW>(); ++q) {
        a = r0 >= v.p[q] ? (uintptr_t)v.b[q] : a;
        inner = inner || (r0 < v.p[q] && r0 + 63u >= v.p[q]);
    }
    return RowBases{a, __ballot(inner)};
}
template <int KW = 1>
__device__ __forceinline__ const uint64_t *row_key_ptr(const BucketView &v, const RowBases &rb, int row, uint32_t i) {
    if ((rb.inner >> row) & 1ull) return bucket_key_ptr<KW>(v, i);  // uniform
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)rb.base, row);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)rb.base >> 32), row);
    return reinterpret_cast<const uint64_t *>((((uint64_t)hi << 32) | lo) + (uintptr_t)i * (8u * KW));
}

constexpr int GB = 8;  // key loads in flight per thread


// ---------------------------------------------------------------------------
// 5a. exact count of one bucket (64-bit keys) in LDS -- the quickSort + RIndex
//     heap merge of extractKXmers (SBKC:540-597).  Two steps on one LDS image:
//       1. dedupe: open addressing (multiplicative hash, linear probing,
//          load <= 1/2) -> distinct keys with multiplicities;
//       2. stable LSD radix sort of the distinct keys only (4-bit digits over
//          the bits that differ inside the bucket, counts as payload).
//     Sorting distinct keys instead of every occurrence divides the sort
//     work by the coverage (4.7x at BASELINE configs[1]).
// ---------------------------------------------------------------------------

constexpr uint32_t HCAP = 2048;                 // keys per LDS bucket
constexpr uint32_t HSLOTS = 2 * HCAP;           // hash slots (load factor <= 1/2)
constexpr uint32_t HSPT = HSLOTS / NT;          // slots per thread in the compaction (16)
constexpr int UIPT = HCAP / NT;                 // distinct keys per thread in the radix sort (8)
constexpr uint32_t RANK_MAX = HCAP - 3 * NT / 2 - 2;  // group-rank sort up to here (upper table half is its scratch)
constexpr uint64_t REDO = ~0ull;                // bucket_unique marker: take the large path
constexpr uint64_t EMPTY_KEY = ~0ull;           // never a canonical k-mer for k <= 32
constexpr uint32_t BLOCK_SPLIT_GROUP = 64;      // block tier: a larger rank group takes the splitter rank

// Weighted keys (64-bit keys with 2k <= WKEY_MAX_BITS): the four bits above the k-mer hold
// weight - 1, so one staged entry stands for 1 .. WKEY_WMAX occurrences of its k-mer (the fold pass,
// k_fold_sc) and a key as the expansion writes it for one.  15 is the largest weight at which a u16
// LDS count cannot overflow in any tier (the largest table holds BIG_HC = 4096 entries).  Every
// reader of staged keys tests EMPTY_KEY first, then splits (key, weight): it hashes, compares and
// ranks on the key alone and adds the weight where an unweighted count adds 1.  2k > 60, or a job
// none of whose pieces was folded (BucketSrc::weighted): no weight field (wsh = 0), every weight 1 --
// the split is then one scalar branch, not the field's arithmetic per key (it cost the unfolded
// configs[1] wave tier 0.1 ms).
struct WKeySpec {
    uint64_t kmask;  // the k-mer's bits
    int wsh;         // the weight field's shift (2k); 0: none
};
__device__ __host__ inline WKeySpec wkey_spec(int k, bool weighted = true) {
    return weighted && 2 * k <= WKEY_MAX_BITS ? WKeySpec{(1ull << (2 * k)) - 1ull, 2 * k} : WKeySpec{~0ull, 0};
}
__device__ __forceinline__ uint64_t wkey_split(uint64_t x, const WKeySpec &ws, uint32_t &w) {
    w = 1u;
    if (ws.wsh == 0) return x;  // uniform
    w += (uint32_t)(x >> ws.wsh);  // nothing lies above the field
    return x & ws.kmask;
}

__device__ __forceinline__ uint32_t hslot(uint64_t key) {
    return (uint32_t)((key * 0x9e3779b97f4a7c15ull) >> 52) & (HSLOTS - 1);  // top 12 bits
}

// HC keys per bucket at most, HS hash slots (a multiple of NT): <2048, 4096> the block
// tier (40 KB of LDS).  STREAM: any number of keys, at most HC of them distinct -- the
// buckets above the block tier (<BIG_HC, BIG_HS> = <4096, 6144>, 60 KB): a bucket of one minimizer-prefix cluster
// holds many copies of few k-mers.  It gives up (REDO, the streaming radix path) once more than
// HC distinct keys or a count of 2^16 - 1 appear; a batch of NT * GB keys adds at most 2048 new
// keys, so the table never fills before the check after each batch.
template <uint32_t HC, uint32_t HS, bool STREAM = false>
__global__ __launch_bounds__(NT) void k_bucket_count64(BucketSrc src, const Bucket *__restrict__ buckets, int k,
                                                       uint64_t *__restrict__ out_keys,
                                                       uint32_t *__restrict__ out_counts, uint64_t *bucket_unique,
                                                       unsigned long long *oversize, uint32_t small_limit,
                                                       int dbg_phase, const uint32_t *__restrict__ list,
                                                       uint32_t skip_le = 0) {
    constexpr uint32_t HSPT_ = HS / NT;              // slots per thread in the compaction
    constexpr int UIPT_ = HC / NT;                    // distinct keys per thread in the radix sort
    // the group-rank sort keeps its counters and its key / count copies in the table's slots
    // above HC, the radix sort its digit counters
    constexpr uint32_t RANK_MAX_ = (HC < HS - HC ? HC : HS - HC) - 3 * NT / 2 - 2;
    static_assert(HC <= 65535 && 2 * HC <= HS + HS / 2 && HS % NT == 0, "u16 counts, load <= 3/4");
    static_assert((HS - HC) * 8 >= 16 * NT * 4 && HC % NT == 0, "radix counters (tile_rank) fit above HC");
    constexpr bool POW2 = (HS & (HS - 1)) == 0;
    constexpr int HBITS = __builtin_ctz(HS);
    __shared__ unsigned long long s_k[HS];
    __shared__ uint16_t s_c[HS];  // counts <= HC fit 16 bits
    __shared__ uint32_t s_tmp[NT / 64];
    // radix counters (U > RANK_MAX only) alias the table's upper half, free once
    // the U <= HCAP distinct keys are compacted to the front
    uint32_t *const s_cnt = reinterpret_cast<uint32_t *>(&s_k[HC]);
    __shared__ uint64_t s_red[2][NT / 64];
    static_assert(!STREAM || HS - HC >= NT * GB, "a batch of new keys leaves the table below full");
    __shared__ uint32_t s_nu, s_ovf;  // STREAM: distinct keys inserted, give-up flag
    __shared__ unsigned long long s_spl[NT];  // splitter rank: sampled keys (2 KB: still 3 workgroups per CU)
    const uint32_t qi = list ? list[blockIdx.x] : blockIdx.x;  // bucket (list: the block tier only)
    const Bucket b = buckets[qi];
    // counted by the mid wave tier (skip_le = 0, every bucket: an empty one -- a cell without keys between
    // two cells that each start a bucket -- must still get its bucket_unique = 0 below)
    if (skip_le && b.n <= skip_le) return;
    const BucketView bv = bucket_view(src, b);
    const WKeySpec ws = wkey_spec(k, src.weighted);
    if (!STREAM && (b.n > HC || b.n > small_limit)) {
        if (threadIdx.x == 0) {
            bucket_unique[qi] = REDO;
            atomicAdd(oversize, 1ull);
        }
        return;
    }
    if (b.n == 0) {
        if (threadIdx.x == 0) bucket_unique[qi] = 0;
        return;
    }
    for (uint32_t s = threadIdx.x; s < HS; s += NT) {
        s_k[s] = EMPTY_KEY;
        s_c[s] = 0;
    }
    if (STREAM && threadIdx.x == 0) s_nu = 0, s_ovf = 0;
    __syncthreads();
    // 1. dedupe: GB independent key loads per thread, then the inserts
    for (uint32_t i0 = 0; i0 < b.n; i0 += NT * GB) {
        if constexpr (STREAM) {
            if (i0) {
                __syncthreads();
                if (s_ovf || s_nu > HC) {
                    if (threadIdx.x == 0) atomicAdd(oversize, 1ull);  // bucket_unique stays REDO
                    return;
                }
            }
        }
        uint64_t kk[GB];
#pragma unroll
        for (int q = 0; q < GB; ++q) {
            const uint32_t i = i0 + q * NT + threadIdx.x;
            kk[q] = i < b.n ? *bucket_key_ptr(bv, i) : EMPTY_KEY;
        }
        if (dbg_phase == 0) {  // timing diagnostic: loads only
            uint64_t acc = 0;
#pragma unroll
            for (int q = 0; q < GB; ++q) acc += kk[q];
            if (acc == 42) out_counts[b.begin] = 1;
            continue;
        }
#pragma unroll
        for (int q = 0; q < GB; ++q) {
            if (kk[q] == EMPTY_KEY) continue;
            uint32_t wt;
            const uint64_t key = wkey_split(kk[q], ws, wt);
            // home slot: the hash's top bits (HS a power of two), else its top 32 bits scaled to HS
            uint32_t s = POW2 ? (uint32_t)((key * 0x9e3779b97f4a7c15ull) >> (64 - HBITS))
                              : (uint32_t)((((key * 0x9e3779b97f4a7c15ull) >> 32) * HS) >> 32);
            for (;;) {
                unsigned long long cur = s_k[s];
                if (cur == EMPTY_KEY) cur = atomicCAS(&s_k[s], EMPTY_KEY, (unsigned long long)key);
                if (cur == EMPTY_KEY || cur == key) {
                    const uint32_t old =
                        atomicAdd(reinterpret_cast<uint32_t *>(&s_c[s & ~1u]), wt << (16 * (s & 1u)));
                    if constexpr (STREAM) {
                        if (cur == EMPTY_KEY) atomicAdd(&s_nu, 1u);
                        if (((old >> (16 * (s & 1u))) & 0xffffu) + wt > 0xffffu) s_ovf = 1u;  // carried: give up
                    }
                    break;
                }
                s = POW2 ? (s + 1) & (HS - 1) : (s + 1 == HS ? 0u : s + 1);
            }
        }
    }
    if (dbg_phase < 99 && threadIdx.x == 0) bucket_unique[qi] = 0;  // timing probes: no output
    if (dbg_phase == 0) return;
    __syncthreads();
    if constexpr (STREAM) {
        if (s_ovf || s_nu > HC) {
            if (threadIdx.x == 0) atomicAdd(oversize, 1ull);
            return;
        }
    }
    if (dbg_phase == 1) return;  // timing diagnostic: gather + dedupe
    // compaction: read own slots (interleaved: slot q*NT + t, so a wave's reads
    // hit consecutive words), then write the distinct keys densely; their order
    // is irrelevant, step 2 sorts them
    uint64_t tk[HSPT_];
    uint16_t tc[HSPT_];
    uint32_t occ = 0;
#pragma unroll
    for (uint32_t q = 0; q < HSPT_; ++q) {
        tk[q] = s_k[q * NT + threadIdx.x];
        tc[q] = s_c[q * NT + threadIdx.x];
        occ += tk[q] != EMPTY_KEY;
    }
    uint32_t U;
    uint32_t u = block_excl_sum<uint32_t>(occ, s_tmp, &U);  // contains a barrier: all reads are done
#pragma unroll
    for (uint32_t q = 0; q < HSPT_; ++q) {
        if (tk[q] != EMPTY_KEY) {
            s_k[u] = tk[q];
            s_c[u] = tc[q];
            ++u;
        }
    }
    __syncthreads();
    if (dbg_phase == 2) return;  // timing diagnostic: + compaction
    // 2. order the U distinct keys.  Their distribution inside a bucket is
    //    spiky (a canonical k-mer often starts with its own minimizer, so keys
    //    of one signature share a 2m-bit prefix), so every key is ranked by its
    //    own thread: keys are grouped by g = (key - lo) >> gsh (at most 256
    //    groups, monotone in the key), and a key's output position is its
    //    group's start plus the number of smaller keys inside the group.  Work
    //    is sum over groups of |g|^2 instead of U^2, and a dense group only
    //    lengthens the loops of the keys that fall into it.
    if (U <= RANK_MAX_) {
        const int sh = 2 * k - src.F;
        const uint64_t lo = (uint64_t)b.c0 << sh;
        const uint32_t ncells = b.c1 - b.c0;
        const int span_bits = (32 - __builtin_clz(ncells)) + sh;
        const int gsh = span_bits > 8 ? span_bits - 8 : 0;
        uint32_t *s_gcnt = reinterpret_cast<uint32_t *>(&s_k[HC]);  // [256] counts, [256] starts, [256] cursors
        uint32_t *s_gst = s_gcnt + NT;
        uint32_t *s_gcur = s_gcnt + 2 * NT;
        s_gcnt[threadIdx.x] = 0;
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < U; i += NT) atomicAdd(&s_gcnt[(uint32_t)((s_k[i] - lo) >> gsh)], 1u);
        __syncthreads();
        if (U > 4 * BLOCK_SPLIT_GROUP) {
            // a dense cluster in one group (the k-mers of a frequent signature share its 2m-bit prefix
            // and land in one group of the uniform cut, where the linear rank costs |group|^2): re-cut
            // the groups at 256 keys sampled from the bucket instead
            uint32_t gmax;
            (void)block_excl_max<uint32_t>(s_gcnt[threadIdx.x], 0u, s_tmp, &gmax);
            if (gmax > BLOCK_SPLIT_GROUP) {
                // samples evenly spaced over the distinct keys (table order: random in the key),
                // bitonic-sorted in LDS
                s_spl[threadIdx.x] = s_k[(uint32_t)(((uint64_t)threadIdx.x * U) / NT)];
                __syncthreads();
                for (uint32_t size = 2; size <= NT; size <<= 1) {
                    for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
                        const uint32_t t = threadIdx.x, o = t ^ stride;
                        if (o > t) {
                            const unsigned long long a = s_spl[t], c = s_spl[o];
                            if ((a > c) == ((t & size) == 0)) s_spl[t] = c, s_spl[o] = a;
                        }
                        __syncthreads();
                    }
                }
                // group of x: the last splitter 1..255 <= x (0 below splitter 1), monotone in x
                auto grp = [&](unsigned long long x) {
                    uint32_t g = 0;
#pragma unroll
                    for (uint32_t st = NT / 2; st >= 1; st >>= 1)
                        if (g + st < NT && s_spl[g + st] <= x) g += st;
                    return g;
                };
                s_gcnt[threadIdx.x] = 0;
                __syncthreads();
                for (uint32_t i = threadIdx.x; i < U; i += NT) atomicAdd(&s_gcnt[grp(s_k[i])], 1u);
                __syncthreads();
                uint32_t tot2;
                const uint32_t st2 = block_excl_sum<uint32_t>(s_gcnt[threadIdx.x], s_tmp, &tot2);
                s_gst[threadIdx.x] = st2;
                s_gcur[threadIdx.x] = st2;
                __syncthreads();
                unsigned long long *s_gk = &s_k[HC + 3 * NT / 2 + 2];
                uint16_t *s_gc = &s_c[HC];
                for (uint32_t i = threadIdx.x; i < U; i += NT) {
                    const unsigned long long kk = s_k[i];
                    const uint32_t p = atomicAdd(&s_gcur[grp(kk)], 1u);
                    s_gk[p] = kk;
                    s_gc[p] = s_c[i];
                }
                __syncthreads();
                for (uint32_t p = threadIdx.x; p < U; p += NT) {
                    const unsigned long long kk = s_gk[p];
                    const uint32_t g = grp(kk);
                    const uint32_t g0 = s_gst[g], g1 = g0 + s_gcnt[g];
                    uint32_t r = g0;
                    for (uint32_t j = g0; j < g1; ++j) r += s_gk[j] < kk;
                    out_keys[b.begin + r] = kk;
                    out_counts[b.begin + r] = s_gc[p];
                }
                if (threadIdx.x == 0) bucket_unique[qi] = U;
                return;
            }
        }
        uint32_t tot;
        const uint32_t st = block_excl_sum<uint32_t>(s_gcnt[threadIdx.x], s_tmp, &tot);
        s_gst[threadIdx.x] = st;
        s_gcur[threadIdx.x] = st;
        __syncthreads();
        // group-ordered copy in the free upper part of the table image
        unsigned long long *s_gk = &s_k[HC + 3 * NT / 2 + 2];
        uint16_t *s_gc = &s_c[HC];
        for (uint32_t i = threadIdx.x; i < U; i += NT) {
            const unsigned long long kk = s_k[i];
            const uint32_t p = atomicAdd(&s_gcur[(uint32_t)((kk - lo) >> gsh)], 1u);
            s_gk[p] = kk;
            s_gc[p] = s_c[i];
        }
        __syncthreads();
        for (uint32_t p = threadIdx.x; p < U; p += NT) {
            const unsigned long long kk = s_gk[p];
            const uint32_t g = (uint32_t)((kk - lo) >> gsh);
            const uint32_t g0 = s_gst[g], g1 = g0 + s_gcnt[g];
            uint32_t r = g0;
            for (uint32_t j = g0; j < g1; ++j) r += s_gk[j] < kk;
            out_keys[b.begin + r] = kk;
            out_counts[b.begin + r] = s_gc[p];
        }
        if (threadIdx.x == 0) bucket_unique[qi] = U;
        return;
    }
    uint64_t key[UIPT_];
    uint32_t cnt[UIPT_];
    const int my0 = threadIdx.x * UIPT_;
    const int nv = max(0, min(UIPT_, (int)U - my0));
    uint64_t kor = 0, kand = ~0ull;
#pragma unroll
    for (int it = 0; it < UIPT_; ++it) {
        if (it < nv) {
            key[it] = s_k[my0 + it];
            cnt[it] = s_c[my0 + it];
            kor |= key[it];
            kand &= key[it];
        } else {
            key[it] = ~0ull;
            cnt[it] = 0;
        }
    }
    {
        const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            kor |= __shfl_xor(kor, d, 64);
            kand &= __shfl_xor(kand, d, 64);
        }
        if (lane == 0) {
            s_red[0][wid] = kor;
            s_red[1][wid] = kand;
        }
        __syncthreads();
        kor = s_red[0][0] | s_red[0][1] | s_red[0][2] | s_red[0][3];
        kand = s_red[1][0] & s_red[1][1] & s_red[1][2] & s_red[1][3];
    }
    const uint64_t diff = kor ^ kand;
    if (diff != 0) {
        const int lo_bit = __builtin_ctzll(diff), hi_bit = 63 - __builtin_clzll(diff);
        for (int sh = lo_bit & ~3; sh <= hi_bit; sh += 4) {
            uint32_t pos[UIPT_], dig[UIPT_];
            tile_rank<uint64_t, UIPT_>(key, nv, sh, s_cnt, s_tmp, pos, dig, nullptr);
#pragma unroll
            for (int it = 0; it < UIPT_; ++it) {
                if (it < nv) {
                    s_k[pos[it]] = key[it];
                    s_c[pos[it]] = cnt[it];
                }
            }
            __syncthreads();
#pragma unroll
            for (int it = 0; it < UIPT_; ++it) {
                if (it < nv) {
                    key[it] = s_k[my0 + it];
                    cnt[it] = s_c[my0 + it];
                }
            }
            __syncthreads();
        }
    }
#pragma unroll
    for (int it = 0; it < UIPT_; ++it) {
        if (it < nv) {
            out_keys[b.begin + my0 + it] = key[it];
            out_counts[b.begin + my0 + it] = cnt[it];
        }
    }
    if (threadIdx.x == 0) bucket_unique[qi] = U;
}

// buckets above the block tier (listed): one 256-thread workgroup with a 6144-slot table each (60 KB
// of LDS: two workgroups per CU; an 8192-slot table of 5888 keys took 84 KB, one workgroup per CU,
// 15.4 ms for the 58 K such buckets of a configs[2] per-GPU load), any number of keys with at
// most BIG_HC distinct; the others keep bucket_unique = REDO (the streaming path) and count into
// *oversize
// (3072 / 5120 slots, 52 KB, three workgroups per CU: profiles/r04c_big_tier_5120_ab.txt)
constexpr uint32_t BIG_HC = 4096, BIG_HS = 6144;
hipError_t launch_bucket_count64_big(const BucketSrc &src, const Bucket *buckets, uint64_t nlist, int k,
                                     uint64_t *out_keys, uint32_t *out_counts, uint64_t *bucket_unique,
                                     unsigned long long *oversize, const uint32_t *list, hipStream_t s) {
    if (!nlist) return hipSuccess;
    k_bucket_count64<BIG_HC, BIG_HS, true><<<(unsigned)nlist, NT, 0, s>>>(src, buckets, k, out_keys, out_counts,
                                                                           bucket_unique, oversize, BIG_HC, 99, list);
    return hipGetLastError();
}

hipError_t launch_bucket_count64(const BucketSrc &src, const Bucket *buckets, uint64_t nbuckets, int k,
                                 uint64_t *out_keys, uint32_t *out_counts, uint64_t *bucket_unique,
                                 unsigned long long *oversize, uint32_t small_limit, int dbg_phase,
                                 const uint32_t *list, hipStream_t s, uint32_t skip_le) {
    if (!nbuckets) return hipSuccess;
    k_bucket_count64<HCAP, HSLOTS><<<(unsigned)nbuckets, NT, 0, s>>>(src, buckets, k, out_keys, out_counts,
                                                                      bucket_unique, oversize, small_limit,
                                                                      dbg_phase, list, skip_le);
    return hipGetLastError();
}


// ---------------------------------------------------------------------------
// 5a'. wave tier (k <= 32): a bucket of at most WCAP keys is counted by one
//      wave with no workgroup barrier (the block kernel above spends most of
//      its time in ~15 barriers per bucket).  Same steps as k_bucket_count64
//      at wave scale: dedupe in a 2*WCAP-slot LDS table (each new key appends
//      its slot to s_list), compaction through the list, then every distinct
//      key is ranked inside its group of the bucket's key range (64 groups,
//      one counter per lane).  Output at the bucket's begin, as the block
//      kernel, for k_bucket_compact.
// ---------------------------------------------------------------------------

// CAP keys per wave bucket (WAVE_BUCKET_CAP or less); SL table slots (2 * CAP, or 1.5 * CAP: the
// table is at most 2/3 full and a wave's LDS image 3/4 of the size -- more waves per CU)
template <uint32_t CAP>
struct WaveCfg {
    static constexpr int KPT = CAP / 64;
    static_assert(CAP == 128 || CAP == 256 || CAP == 512 || CAP == 1024, "CAP must be 128 .. 1024");
};

// home slot in [0, SL): the top 32 bits of a multiplicative hash scaled to SL (for SL a power of
// two: its top log2(SL) bits)
template <uint32_t SL>
__device__ __forceinline__ uint32_t wslot(uint64_t key) {
    const uint32_t h = (uint32_t)((key * 0x9e3779b97f4a7c15ull) >> 32);
    return (uint32_t)(((uint64_t)h * SL) >> 32);
}

// LDS writes of this wave visible to its later LDS reads (no workgroup
// barrier).  A wave's LDS operations complete in order, so waiting for its
// LDS counter suffices; a wavefront-scope fence would also wait for every
// outstanding global load (vmcnt(0)), i.e. for the prefetched next bucket.
__device__ __forceinline__ void wave_lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// One bucket's keys (<= CAP), KPT per lane; MS: from the staged pieces' arrays (src.np > 0)
template <uint32_t CAP, bool MS, int WKPT = WaveCfg<CAP>::KPT>
__device__ __forceinline__ void wave_bucket_load(const BucketSrc &src, const Bucket &b, const PieceStarts &ps,
                                                 bool mine, uint64_t (&kk)[WKPT], const uint64_t *dummy) {
    // every lane of every bucket loads (lanes past the bucket, and buckets not counted here, from
    // `dummy`, a readable address): loads that are never branched over let the first bucket's count
    // wait for its own keys only (vmcnt(n), not vmcnt(0))
    BucketView v{};
    RowBases rb{};
    if constexpr (MS) {
        if (mine) {  // uniform
            v = src.starts ? bucket_view_starts(src, ps) : bucket_view(src, b);
            rb = row_bases(v);
        }
    }
#pragma unroll
    for (int j = 0; j < WKPT; ++j) {
        const uint32_t i = j * 64 + (threadIdx.x & 63);
        const bool ok = mine && i < b.n;
        // the row's address without a branch on `ok` (an exec-mask round per row), then the select
        const uint64_t *pa = MS ? row_key_ptr(v, rb, j, i) : src.keys + b.begin + i;
        const uint64_t *a = ok ? pa : dummy;
        const uint64_t x = ldg_nt<uint64_t>(a);
        kk[j] = ok ? x : EMPTY_KEY;
    }
}

template <uint32_t CAP, uint32_t SL>
struct WaveLds {
    static_assert(SL >= CAP && SL % 8 == 0, "the table holds every distinct key; cleared 8 counts at a time");
    // the rank's group words (256 for CAP > 128, else 64) live in the dead table's slots above CAP
    static_assert((SL - CAP) * 8 >= (CAP > 128 ? 1024u : 256u), "group words above CAP");
    unsigned long long k[SL];  // the table; then the distinct keys in group order
    uint16_t c[SL];            // their counts
    uint16_t list[CAP];
};

#ifdef FK_PROBES
__device__ unsigned long long g_rank_probe[4];
hipError_t rank_probe_read(unsigned long long *out4, bool reset) {
    hipError_t e = hipMemcpyFromSymbol(out4, HIP_SYMBOL(g_rank_probe), 32, 0, hipMemcpyDeviceToHost);
    if (e == hipSuccess && reset) {
        const unsigned long long z[4] = {0, 0, 0, 0};
        e = hipMemcpyToSymbol(HIP_SYMBOL(g_rank_probe), z, 32, 0, hipMemcpyHostToDevice);
    }
    return e;
}
#endif

// 3. the rank of U distinct keys (key i = j * 64 + lane in tk, counts tc) inside G groups of the key
//    range [lo, lo + 2^span_bits): each key with its count written at out_keys / out_counts + begin +
//    its rank.  LDS: s_gk / s_gc hold the group-ordered copy (>= U entries, dead before the call),
//    s_grp the group words (256), s_scnt 128 words.
template <uint32_t CAP, int WKPT>
__device__ __forceinline__ void wave_rank64(unsigned long long *s_gk, uint16_t *s_gc, uint32_t *s_grp, uint32_t *s_scnt,
                                            uint32_t U, const uint64_t (&tk)[WKPT], const uint16_t (&tc)[WKPT],
                                            uint64_t lo, int span_bits, uint64_t begin,
                                            uint64_t *__restrict__ out_keys, uint32_t *__restrict__ out_counts) {
    const int lane = threadIdx.x & 63;
    // 3. rank inside G groups of the key range [lo, lo + 2^span_bits): G = 64, or 256 when the
    //    bucket holds more than 128 distinct keys (mostly distinct k-mers: a key's rank loop runs
    //    over its group, ~U / G keys)
    const bool wide = CAP > 128 && U > 128;  // uniform
    const int gbits = wide ? 8 : 6;
    const int gsh = span_bits > gbits ? span_bits - gbits : 0;
    // per group one word: its key count << 16 | its cursor (the group's start, then its end once
    // the keys are scattered) -- one read gives a key both bounds of its group
    wave_lds_sync();  // the table reads above are done before the table is overwritten below
    if (wide)
        reinterpret_cast<uint4 *>(s_grp)[lane] = make_uint4(0, 0, 0, 0);
    else
        s_grp[lane] = 0;
    wave_lds_sync();
#pragma unroll
    for (int j = 0; j < WKPT; ++j)
        if (j * 64 + lane < (int)U) atomicAdd(&s_grp[(uint32_t)((tk[j] - lo) >> gsh)], 1u << 16);
    wave_lds_sync();
    if (wide) {  // lane l owns groups 4l .. 4l + 3
        const uint4 c = reinterpret_cast<const uint4 *>(s_grp)[lane];
        const uint32_t cx = c.x >> 16, cy = c.y >> 16, cz = c.z >> 16, t = cx + cy + cz + (c.w >> 16);
        const uint32_t base = wave_incl_sum<uint32_t>(t) - t;
        reinterpret_cast<uint4 *>(s_grp)[lane] =
            make_uint4(c.x | base, c.y | (base + cx), c.z | (base + cx + cy), c.w | (base + cx + cy + cz));
    } else {
        const uint32_t c = s_grp[lane], gc = c >> 16;
        s_grp[lane] = c | (wave_incl_sum<uint32_t>(gc) - gc);
    }
    wave_lds_sync();
#pragma unroll
    for (int j = 0; j < WKPT; ++j) {
        if (j * 64 + lane < (int)U) {
            const uint32_t p = atomicAdd(&s_grp[(uint32_t)((tk[j] - lo) >> gsh)], 1u) & 0xffffu;
            s_gk[p] = tk[j];
            s_gc[p] = tc[j];
        }
    }
    wave_lds_sync();
#ifdef FK_PROBES
    uint32_t it = 0, wall = 0;
#endif
    // 3b. groups of more than RANK_BIG keys (a cluster: keys sharing bits below the group's, e.g. a
    //     minimizer's k-mers that start with it, whose rank loops would run over the whole cluster)
    //     are ranked by a second cut: 64 sub-groups by the 6 bits below the group's own common prefix
    //     (found from the OR of its keys' XOR with its first), counted, scattered in place, then the
    //     rank loop over a key's sub-group.  One group at a time, the wave's lanes over its keys.
    constexpr uint32_t RANK_BIG = 24;
    static_assert(CAP >= 256, "64 + 64 sub-group counters");
    uint32_t *s_scur = s_scnt + 64;
    const int ncomp = wide ? 4 : 1;
    for (int comp = 0; comp < ncomp; ++comp) {
        const uint32_t mine = (wide ? s_grp[4 * lane + comp] : s_grp[lane]) >> 16;
        uint64_t bm = __ballot(mine > RANK_BIG);
        while (bm) {  // uniform
            const uint32_t g = (uint32_t)(wide ? 4 * __builtin_ctzll(bm) + comp : __builtin_ctzll(bm));
            bm &= bm - 1;
            const uint32_t gv = s_grp[g], cnt = gv >> 16, g0 = (gv & 0xffffu) - cnt;
            const unsigned long long x0 = s_gk[g0];
            uint64_t gk[WKPT];
            uint16_t gcv[WKPT];
            unsigned long long orx = 0;
#pragma unroll
            for (int j = 0; j < WKPT; ++j) {
                const uint32_t i = j * 64 + lane;
                if (i < cnt) {
                    gk[j] = s_gk[g0 + i];
                    gcv[j] = s_gc[g0 + i];
                    orx |= gk[j] ^ x0;
                }
            }
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) orx |= (unsigned long long)__shfl_xor((long long)orx, d, 64);
            const int hb = 63 - __builtin_clzll(orx | 1ull);  // the group's keys agree above bit hb
            const int ssh = hb >= 5 ? hb - 5 : 0;
            s_scnt[lane] = 0;
            wave_lds_sync();
#pragma unroll
            for (int j = 0; j < WKPT; ++j)
                if (j * 64 + lane < (int)cnt) atomicAdd(&s_scnt[(uint32_t)(gk[j] >> ssh) & 63u], 1u);
            wave_lds_sync();
            const uint32_t sc = s_scnt[lane];
            s_scur[lane] = wave_incl_sum<uint32_t>(sc) - sc;
            wave_lds_sync();
#pragma unroll
            for (int j = 0; j < WKPT; ++j) {
                if (j * 64 + lane < (int)cnt) {
                    const uint32_t pos = g0 + atomicAdd(&s_scur[(uint32_t)(gk[j] >> ssh) & 63u], 1u);
                    s_gk[pos] = gk[j];
                    s_gc[pos] = gcv[j];
                }
            }
            wave_lds_sync();
#pragma unroll
            for (int j = 0; j < WKPT; ++j) {
                if (j * 64 + lane < (int)cnt) {
                    const uint32_t sb = (uint32_t)(gk[j] >> ssh) & 63u;
                    const uint32_t s1 = g0 + s_scur[sb], s0 = s1 - s_scnt[sb];
                    uint32_t r = s0;
                    for (uint32_t t = s0; t < s1; ++t) r += s_gk[t] < gk[j];
                    out_keys[begin + r] = gk[j];
                    out_counts[begin + r] = gcv[j];
#ifdef FK_PROBES
                    it += s1 - s0;
#endif
                }
            }
            wave_lds_sync();  // the sub-group counters are reused by the next group
        }
    }
#if defined(FK_W64_STOP) && FK_W64_STOP == 3  // phase probe: stop before the final rank loop
    return;
#endif
    for (uint32_t p = lane; p < U; p += 64) {
        const unsigned long long kx = s_gk[p];
        const uint32_t g = (uint32_t)((kx - lo) >> gsh);
        const uint32_t gv = s_grp[g], n = gv >> 16;
        if (n > RANK_BIG) continue;  // ranked above
        const uint32_t g1 = gv & 0xffffu, g0 = g1 - n;  // the cursor ends at the group's end
        // four members per round, read together (the loop is bound by its LDS round trips, and the
        // wave runs as long as its largest group); reads past the group stay inside the table
        uint32_t r = g0;
        for (uint32_t j = g0; j < g1; j += 4) {
            const unsigned long long a0 = s_gk[j], a1 = s_gk[j + 1], a2 = s_gk[j + 2], a3 = s_gk[j + 3];
            r += (uint32_t)(a0 < kx) + (uint32_t)(j + 1 < g1 && a1 < kx) + (uint32_t)(j + 2 < g1 && a2 < kx) +
                 (uint32_t)(j + 3 < g1 && a3 < kx);
        }
        out_keys[begin + r] = kx;
        out_counts[begin + r] = s_gc[p];
#ifdef FK_PROBES
        it += g1 - g0;
        uint32_t w = g1 - g0;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) w = max(w, (uint32_t)__shfl_xor((int)w, d, 64));
        wall += w;
#endif
    }
#ifdef FK_PROBES
    it = wave_incl_sum<uint32_t>(it);
    if (lane == 63) {
        atomicAdd(&g_rank_probe[0], (unsigned long long)it);
        atomicAdd(&g_rank_probe[1], (unsigned long long)U);
        atomicAdd(&g_rank_probe[2], 1ull);
        atomicAdd(&g_rank_probe[3], (unsigned long long)wall);
    }
#endif
}

// count n <= CAP keys (held in kk) with the calling wave: the distinct keys with their counts at
// out_keys / out_counts + begin, their number in uniq[q] -- ascending (ORD), or in the table's order
// of first insertion (useHT: extractKXmersHT writes its hash map's iteration order, SBKC:723-734, so
// the rank below is skipped).  Every key lies in [lo, lo + 2^span_bits) (the rank's group cut).
// Returns the number of distinct keys (wave-uniform); uniq may be null.  NROW > WKPT rows of keys
// (the mid tier's up to 1024 keys on the 512-key table): the count gives up -- returns ~0u, writes
// nothing -- once more than CAP distinct keys appear (checked before each row: the table keeps
// SL - CAP >= 64 free slots for the row's new keys).
// WT = false (the main wave tier of a job without a folded piece, the kernel every key of such a job
// passes through): the weight split is compiled out -- its key mask and branch cost the unfolded
// configs[2] load 0.4 ms per step
template <uint32_t CAP, uint32_t SL, bool ORD = true, int WKPT = WaveCfg<CAP>::KPT, int NROW = WKPT, bool WT = true>
__device__ __forceinline__ uint32_t wave_count_keys(WaveLds<CAP, SL> &w, uint64_t begin, uint32_t n, uint64_t lo,
                                                int span_bits, uint64_t q, const uint64_t (&kk)[NROW],
                                                const WKeySpec ws, uint64_t *__restrict__ out_keys,
                                                uint32_t *__restrict__ out_counts, uint64_t *__restrict__ uniq) {
    const int lane = threadIdx.x & 63;
    unsigned long long *s_k = w.k;
    uint16_t *s_c = w.c;
    uint16_t *s_list = w.list;
    if (n == 0) {
        if (lane == 0 && uniq) uniq[q] = 0;
        return 0;
    }
    {
        ulonglong2 *k2 = reinterpret_cast<ulonglong2 *>(s_k);
#pragma unroll
        for (uint32_t r = 0; r < (SL / 2 + 63) / 64; ++r)
            if (r * 64 + lane < SL / 2) k2[r * 64 + lane] = make_ulonglong2(EMPTY_KEY, EMPTY_KEY);
        uint4 *c4 = reinterpret_cast<uint4 *>(s_c);
#pragma unroll
        for (uint32_t r = 0; r < (SL / 8 + 63) / 64; ++r)
            if (r * 64 + lane < SL / 8) c4[r * 64 + lane] = make_uint4(0, 0, 0, 0);
    }
    wave_lds_sync();
    // 1. dedupe: the lane's keys are inserted one after another, every probe a
    //    compare-and-swap (an occupied slot returns its key: one LDS round trip
    //    per probe and a short loop; round 5's form, the first probes
    //    read together and a swap only on an empty slot, was slower
    //    at every load measured: configs[2] wave tier 24.2 -> 21.4 ms, configs[1]
    //    step 22.3 -> 22.1 ms, profiles/r06i_ab.txt).  The list of new keys'
    //    slots is built from ballots (the wave owns the bucket: no atomic
    //    counter).
    static_assert(NROW == WKPT || (NROW > WKPT && SL - CAP >= 64), "a row's new keys fit above CAP");
    uint32_t sl[NROW];
#pragma unroll
    for (int j = 0; j < NROW; ++j) sl[j] = wslot<SL>(WT ? kk[j] & ws.kmask : kk[j]);
    uint32_t U = 0;
#pragma unroll
    for (int j = 0; j < NROW; ++j) {
        bool over = false;  // uniform: more than CAP distinct keys so far (given up below)
        if constexpr (NROW > WKPT) over = U > CAP;
        const uint64_t x = over ? EMPTY_KEY : kk[j];
        bool fresh = false;
        if (x != EMPTY_KEY) {
            uint32_t wt = 1u;
            uint64_t key = x;
            if constexpr (WT) key = wkey_split(x, ws, wt);
            uint32_t s = sl[j];
            for (;;) {  // every probe a compare-and-swap
                const unsigned long long prev = atomicCAS(&s_k[s], EMPTY_KEY, (unsigned long long)key);
                fresh = prev == EMPTY_KEY;
                if (fresh || prev == key) break;
                s = s + 1 == SL ? 0u : s + 1;
            }
            atomicAdd(reinterpret_cast<uint32_t *>(&s_c[s & ~1u]), wt << (16 * (s & 1u)));
            sl[j] = s;
        }
        const uint64_t m = __ballot(fresh);
        if (fresh) {
            const uint32_t at = U + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            if (NROW == WKPT || at < CAP) s_list[at] = (uint16_t)sl[j];
        }
        U += (uint32_t)__popcll(m);
    }
    wave_lds_sync();
    if constexpr (NROW > WKPT) {
        if (U > CAP) return ~0u;  // uniform: more distinct keys than the rank holds
    }
#if defined(FK_W64_STOP) && FK_W64_STOP == 1  // phase probe (measurement builds only): stop after the dedupe
    if (lane == 0 && uniq) uniq[q] = U;
    return U;
#endif
    // 2. the distinct keys and their counts into registers through the slot list (key i = j * 64 +
    //    lane); the table is dead after these reads
    uint64_t tk[WKPT];
    uint16_t tc[WKPT];
#pragma unroll
    for (int j = 0; j < WKPT; ++j) {
        const uint32_t i = j * 64 + lane;
        if (i < U) {
            const uint32_t s = s_list[i];
            tk[j] = s_k[s];
            tc[j] = s_c[s];
        }
    }
#if defined(FK_W64_STOP) && FK_W64_STOP == 2  // phase probe: stop after the read-back
    {
        uint64_t x = 0;
#pragma unroll
        for (int j = 0; j < WKPT; ++j) x ^= (j * 64 + lane < (int)U) ? tk[j] + tc[j] : 0ull;
        if (x == 0x0123456789abcdefull) out_counts[0] = 1u;  // keeps the reads
        if (lane == 0 && uniq) uniq[q] = U;
        wave_lds_sync();
        return U;
    }
#endif
    if constexpr (!ORD) {
#pragma unroll
        for (int j = 0; j < WKPT; ++j) {
            const uint32_t i = j * 64 + lane;
            if (i < U) {
                out_keys[begin + i] = tk[j];
                out_counts[begin + i] = tc[j];
            }
        }
        if (lane == 0 && uniq) uniq[q] = U;
        wave_lds_sync();  // LDS reads of this bucket done before the table is reused
        return U;
    }
    // 3. rank: the group words above every slot of the group-ordered copy, which goes over the dead
    //    table; the second cut's counters in the dead slot list
    wave_rank64<CAP, WKPT>(s_k, s_c, reinterpret_cast<uint32_t *>(&s_k[CAP]), reinterpret_cast<uint32_t *>(s_list),
                           U, tk, tc, lo, span_bits, begin, out_keys, out_counts);
    if (lane == 0 && uniq) uniq[q] = U;
    wave_lds_sync();  // LDS reads of this bucket done before the table is reused
    return U;
}

// count one bucket (cells [c0, c1) of its bin) of <= CAP keys with the calling wave
template <uint32_t CAP, uint32_t SL, bool ORD = true, bool WT = true, int WKPT = WaveCfg<CAP>::KPT>
__device__ __forceinline__ void wave_count_bucket(WaveLds<CAP, SL> &w, const Bucket &b, uint64_t q,
                                                  const uint64_t (&kk)[WKPT], int k, int F, const WKeySpec ws,
                                                  uint64_t *__restrict__ out_keys, uint32_t *__restrict__ out_counts,
                                                  uint64_t *__restrict__ bucket_unique) {
    const int sh = 2 * k - F;
    const int span_bits = b.n ? (32 - __builtin_clz(b.c1 - b.c0)) + sh : 0;
    wave_count_keys<CAP, SL, ORD, WKPT, WKPT, WT>(w, b.begin, b.n, (uint64_t)b.c0 << sh, span_bits, q, kk, ws,
                                        out_keys, out_counts, bucket_unique);
}

// BPW buckets per wave: all their keys are loaded up front, so a wave waits
// for HBM once per BPW buckets (waves per CU are LDS-bound).  list: bucket
// indices (the wave tier of the buckets not counted by k_fine_sc_count), or
// null for buckets 0..nbuckets-1.
template <int BPW, uint32_t CAP, uint32_t SL, bool MS = false, bool ORD = true, bool WT = true>
__global__ __launch_bounds__(64) void k_bucket_count64_wave(BucketSrc src,
                                                            const Bucket *__restrict__ buckets, uint64_t nbuckets,
                                                            int k, uint64_t *__restrict__ out_keys,
                                                            uint32_t *__restrict__ out_counts,
                                                            uint64_t *__restrict__ bucket_unique,
                                                            const uint32_t *__restrict__ list) {
    constexpr int WKPT = WaveCfg<CAP>::KPT;
    __shared__ __attribute__((aligned(16))) WaveLds<CAP, SL> w;
    const uint64_t q0 = (uint64_t)blockIdx.x * BPW;
    Bucket b[BPW];
    bool mine[BPW];
    uint64_t qq[BPW];
    uint64_t kk[BPW][WKPT];
    const uint64_t *dummy = reinterpret_cast<const uint64_t *>(buckets);
#pragma unroll
    for (int t = 0; t < BPW; ++t) {
        const uint64_t i = q0 + t;
        qq[t] = i < nbuckets ? (list ? (uint64_t)list[i] : i) : 0;
        if (i < nbuckets) b[t] = buckets[qq[t]];
        PieceStarts ps{};
        if constexpr (MS)
            if (src.starts && i < nbuckets) ps = src.starts[qq[t]];
        mine[t] = i < nbuckets && b[t].n <= CAP;  // larger: block tier / large path
        wave_bucket_load<CAP, MS>(src, b[t], ps, mine[t], kk[t], dummy);
    }
#if defined(FK_W64_STOP) && FK_W64_STOP == 0  // phase probe: the key loads only
    if (!list) {
#pragma unroll
        for (int t = 0; t < BPW; ++t) {
            uint64_t x = 0;
#pragma unroll
            for (int j = 0; j < WKPT; ++j) x ^= kk[t][j];
            if ((threadIdx.x & 63) == 0 && bucket_unique && mine[t]) bucket_unique[qq[t]] = 0;
            if (x == 0x0123456789abcdefull) out_counts[0] = 1u;  // keeps the loads
        }
        return;
    }
#endif
#pragma unroll
    for (int t = 0; t < BPW; ++t)
        if (mine[t])
            wave_count_bucket<CAP, SL, ORD, WT>(w, b[t], qq[t], kk[t], k, src.F, wkey_spec(k, src.weighted), out_keys,
                                            out_counts, bucket_unique);
}

// greedy bucket cut per bin: consecutive cells are packed while the bucket
// stays <= cap keys; a cell above cap is a bucket of its own; with period_bits
// >= 0 a bucket also starts at every multiple of 2^period_bits cells (so no
// bucket spans two super-cells).  One workgroup per bin; each lane of wave 0
// packs its 1/64 of the bin's cells (a cut at every segment start costs ~10%
// more buckets than one sequential pass); all FLAGS_NT threads stage the
// cell totals through LDS and store the flags.
constexpr int FLAGS_NT = 256;
__global__ __launch_bounds__(FLAGS_NT) void k_bucket_flags_greedy(const uint64_t *__restrict__ cell_total, int F,
                                                            uint32_t cap, int period_bits,
                                                            uint32_t *__restrict__ flags) {
    extern __shared__ uint32_t s_t[];
    const uint32_t ncell = 1u << F;
    const uint32_t pmask = period_bits >= 0 ? (1u << period_bits) - 1u : 0xffffffffu;
    const uint64_t *t = cell_total + ((uint64_t)blockIdx.x << F);
    uint32_t *f = flags + ((uint64_t)blockIdx.x << F);
    for (uint32_t c = threadIdx.x; c < ncell; c += FLAGS_NT) {
        const uint64_t v = t[c];
        s_t[c] = v > 0xffffffffull ? 0xffffffffu : (uint32_t)v;
    }
    __syncthreads();
    if (threadIdx.x < 64) {
        const uint32_t seg = (ncell + 63) / 64;
        const uint32_t c0 = threadIdx.x * seg, c1 = min(c0 + seg, ncell);
        uint64_t acc = 0;
        bool prev_big = false;
        for (uint32_t c = c0; c < c1; ++c) {
            const uint32_t v = s_t[c];
            const bool big = v > cap;
            const bool cut = c == c0 || (c & pmask) == 0 || big || prev_big || acc + v > cap;
            acc = cut ? v : acc + v;
            prev_big = big;
            s_t[c] = cut;  // own segment only
        }
    }
    __syncthreads();
    for (uint32_t c = threadIdx.x; c < ncell; c += FLAGS_NT) f[c] = s_t[c];
}

// tiers: n <= wave_cap the wave kernel (every bucket, unlisted), <= block_cap
// the block kernel (listed), else the large path (REDO, listed).
// lists[0, nb) block tier, lists[nb, 2 nb) large; counts[0..1] their lengths.
constexpr int TIER_IPT = 8;  // buckets per thread: one pair of list atomics per NT * TIER_IPT buckets
__global__ __launch_bounds__(NT) void k_bucket_tiers(const Bucket *__restrict__ buckets, uint64_t nb,
                                                     uint32_t wave_cap, uint32_t block_cap,
                                                     uint64_t *__restrict__ bucket_unique,
                                                     uint32_t *__restrict__ block_list,
                                                     uint32_t *__restrict__ large_list, unsigned int *counts /*[2]*/,
                                                     unsigned long long *listed_keys) {
    __shared__ uint32_t s_tmp[NT / 64];
    __shared__ uint32_t s_base[2];
    const uint64_t i0 = ((uint64_t)blockIdx.x * NT + threadIdx.x) * TIER_IPT;
    uint32_t n[TIER_IPT];
#pragma unroll
    for (int t = 0; t < TIER_IPT; ++t) n[t] = i0 + t < nb ? buckets[i0 + t].n : 0u;
    uint32_t mine = 0;  // (block << 16) | large, <= TIER_IPT each
    unsigned long long keys = 0;
#pragma unroll
    for (int t = 0; t < TIER_IPT; ++t) {
        const bool is_block = n[t] > wave_cap && n[t] <= block_cap, is_large = n[t] > block_cap;
        if (is_large) bucket_unique[i0 + t] = REDO;
        mine += ((uint32_t)is_block << 16) | (uint32_t)is_large;
        if (n[t] > wave_cap) keys += n[t];
    }
    // the listed keys: one atomic per workgroup (one per wave serialized ~16 K atomics on one address
    // at the configs[2] load)
    __shared__ unsigned long long s_keys[NT / 64];
    keys = wave_incl_sum<unsigned long long>(keys);
    if ((threadIdx.x & 63) == 63) s_keys[threadIdx.x >> 6] = keys;
    uint32_t tot;
    // one atomic per workgroup and list: (block << 16) | large packed in one scan
    uint32_t off = block_excl_sum<uint32_t>(mine, s_tmp, &tot);  // its barrier orders s_keys too
    if (threadIdx.x == 0) {
        s_base[0] = (tot >> 16) ? atomicAdd(&counts[0], tot >> 16) : 0u;
        s_base[1] = (tot & 0xffffu) ? atomicAdd(&counts[1], tot & 0xffffu) : 0u;
        unsigned long long kt = 0;
#pragma unroll
        for (int w = 0; w < NT / 64; ++w) kt += s_keys[w];
        if (kt) atomicAdd(listed_keys, kt);
    }
    __syncthreads();
    if (!mine) return;
    uint32_t ob = s_base[0] + (off >> 16), ol = s_base[1] + (off & 0xffffu);
#pragma unroll
    for (int t = 0; t < TIER_IPT; ++t) {
        if (n[t] > wave_cap && n[t] <= block_cap) block_list[ob++] = (uint32_t)(i0 + t);
        if (n[t] > block_cap) large_list[ol++] = (uint32_t)(i0 + t);
    }
}

hipError_t launch_bucket_flags_greedy(const uint64_t *cell_total, uint32_t nlbins, int F, uint32_t cap,
                                      int period_bits, uint32_t *flags, hipStream_t s) {
    if (!nlbins) return hipSuccess;
    hipError_t e = part_lds_attr((const void *)k_bucket_flags_greedy, (size_t)4 << F);  // up to 128 KB at F = 15
    if (e != hipSuccess) return e;
    k_bucket_flags_greedy<<<nlbins, FLAGS_NT, (size_t)4 << F, s>>>(cell_total, F, cap, period_bits, flags);
    return hipGetLastError();
}

hipError_t launch_bucket_tiers(const Bucket *buckets, uint64_t nb, uint32_t wave_cap, uint32_t block_cap,
                               uint64_t *bucket_unique, uint32_t *lists, unsigned int *counts,
                               unsigned long long *listed_keys, hipStream_t s) {
    if (!nb) return hipSuccess;
    k_bucket_tiers<<<(unsigned)((nb + (uint64_t)NT * TIER_IPT - 1) / ((uint64_t)NT * TIER_IPT)), NT, 0, s>>>(
        buckets, nb, wave_cap, block_cap, bucket_unique, lists, lists + nb, counts, listed_keys);
    return hipGetLastError();
}

// Every bucket of <= WAVE_BUCKET_CAP keys: two buckets per wave (their keys loaded up front), WAVE_SLOTS-slot
// tables (at most 2/3 full: 16 waves per CU against 13 with 1024 slots; 128 / 256-key buckets, one or
// four buckets per wave and 1024 slots measured slower, DESIGN.md 4 "Count")
hipError_t launch_bucket_count64_wave(const BucketSrc &src, const Bucket *buckets, uint64_t nbuckets, int k,
                                      uint64_t *out_keys, uint32_t *out_counts, uint64_t *bucket_unique,
                                      const uint32_t *list, hipStream_t s, bool ordered) {
    if (!nbuckets) return hipSuccess;
    const unsigned grid = (unsigned)((nbuckets + 1) / 2);
#define FK_W64T(MS_, ORD_, WT_)                                                                                 \
    k_bucket_count64_wave<2, WAVE_BUCKET_CAP, WAVE_SLOTS, MS_, ORD_, WT_><<<grid, 64, 0, s>>>(                 \
        src, buckets, nbuckets, k, out_keys, out_counts, bucket_unique, list)
#define FK_W64(MS_, ORD_)                    \
    do {                                     \
        if (src.weighted)                    \
            FK_W64T(MS_, ORD_, true);        \
        else                                 \
            FK_W64T(MS_, ORD_, false);       \
    } while (0)
    if (src.np > 0 && ordered)
        FK_W64(true, true);
    else if (src.np > 0)
        FK_W64(true, false);
    else if (ordered)
        FK_W64(false, true);
    else
        FK_W64(false, false);
#undef FK_W64
#undef FK_W64T
    return hipGetLastError();
}

// The block tier's buckets of at most WAVE_MID_CAP keys (listed, all above WAVE_BUCKET_CAP): one wave
// each, 16 keys per lane, a WAVE_MID_SLOTS-slot table (1280 slots, 14.6 KB of LDS per wave).  They are minimizer-prefix
// clusters, whose rank the second cut in wave_count_keys handles; the block kernel skips them.
hipError_t launch_bucket_count64_wave_mid(const BucketSrc &src, const Bucket *buckets, const uint32_t *list,
                                          uint64_t nlist, int k, uint64_t *out_keys, uint32_t *out_counts,
                                          uint64_t *bucket_unique, hipStream_t s, bool ordered) {
    if (!nlist) return hipSuccess;
#define FK_W64M(MS_, ORD_)                                                                                  \
    k_bucket_count64_wave<1, WAVE_MID_CAP, WAVE_MID_SLOTS, MS_, ORD_><<<(unsigned)nlist, 64, 0, s>>>( \
        src, buckets, nlist, k, out_keys, out_counts, bucket_unique, list)
    if (src.np > 0 && ordered)
        FK_W64M(true, true);
    else if (src.np > 0)
        FK_W64M(true, false);
    else if (ordered)
        FK_W64M(false, true);
    else
        FK_W64M(false, false);
#undef FK_W64M
    return hipGetLastError();
}



// The mid tier's buckets (513 .. 1024 keys) as 2 or 3 key ranges counted in order by the wave tier's
// code (k_bucket_count64_parts): the range bounds are quantiles of a 64-key sample sorted across the
// wave; each range's keys are gathered (from L2: the bucket was just read) into LDS, read back 8 per
// lane, and counted with the 640-slot table at the output after the previous ranges' distinct keys.
// The wave tier's LDS image (7.4 KB) instead of the 1024-key table's 14.8 KB: twice the waves per CU.
// A bucket whose range exceeds 512 keys (a k-mer repeated that often) is listed for the 1024-key
// kernel (fb / fb_count).
template <bool MS, bool ORD>
__global__ __launch_bounds__(64) void k_bucket_count64_parts(BucketSrc src, const Bucket *__restrict__ buckets,
                                                             const uint32_t *__restrict__ list, int k,
                                                             uint64_t *__restrict__ out_keys,
                                                             uint32_t *__restrict__ out_counts,
                                                             uint64_t *__restrict__ bucket_unique,
                                                             uint32_t *__restrict__ fb, unsigned int *fb_count) {
    constexpr uint32_t CAP = WAVE_BUCKET_CAP, SL = WAVE_SLOTS;
    constexpr int WKPT = WaveCfg<CAP>::KPT, R = 2 * WKPT;  // R keys per lane cover WAVE_MID_CAP
    static_assert(R * 64 == WAVE_MID_CAP && SL >= CAP, "two rounds of the wave tier's keys per lane");
    __shared__ __attribute__((aligned(16))) WaveLds<CAP, SL> w;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t q = list[blockIdx.x];
    const Bucket b = buckets[q];
    BucketView v{};
    if constexpr (MS) v = src.starts ? bucket_view_starts(src, src.starts[q]) : bucket_view(src, b);
    else v = bucket_view(src, b);
    const uint32_t n = b.n;
    const uint64_t *klast = bucket_key_ptr(v, n - 1);
    const RowBases rb = row_bases(v);  // the 16 rows' piece bases, once
    auto key_at = [&](uint32_t row0, uint32_t i) {
        const uint64_t *pa = row_key_ptr(v, rb, (int)(row0 >> 6), i);
        return ldg_nt<uint64_t>(i < n ? pa : klast);
    };
    // 1. a sample of 64 keys, one per lane, sorted across the wave (bitonic, ascending by lane)
    const WKeySpec ws = wkey_spec(k, src.weighted);  // the sample, the sizes and the ranges on the k-mer alone
    unsigned long long x = *bucket_key_ptr(v, (uint32_t)(((uint64_t)lane * n) >> 6)) & ws.kmask;
#pragma unroll
    for (uint32_t kk = 2; kk <= 64; kk <<= 1) {
#pragma unroll
        for (uint32_t j = kk >> 1; j > 0; j >>= 1) {
            const unsigned long long y = (unsigned long long)__shfl_xor((long long)x, (int)j, 64);
            const bool up = (lane & kk) == 0, low = (lane & j) == 0;
            x = (low == up) ? (x < y ? x : y) : (x > y ? x : y);
        }
    }
    // 2. P ranges: (sp[p - 1], sp[p]], splitters at the sample's P-quantiles
    const uint32_t P = n <= 768 ? 2u : 3u;
    const unsigned long long sp0 = (unsigned long long)__shfl((long long)x, (int)(64 / P) - 1, 64);
    const unsigned long long sp1 = (unsigned long long)__shfl((long long)x, (int)(2 * 64 / P) - 1, 64);
    auto range_of = [&](unsigned long long key) -> uint32_t {
        return (key > sp0 ? 1u : 0u) + (P == 3 && key > sp1 ? 1u : 0u);
    };
    // the bucket's keys in registers (16 per lane), read once for the size pass and every gather
    uint64_t kr[R];
#pragma unroll
    for (int r = 0; r < R; ++r) kr[r] = key_at(r * 64, r * 64 + lane);
    // 3. the ranges' sizes; one above the wave tier's cap leaves the bucket to the 1024-key kernel
    uint32_t c0 = 0, c1 = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint32_t i = r * 64 + lane;
        const unsigned long long key = kr[r] & ws.kmask;
        const uint32_t g = range_of(key);
        c0 += (i < n && g == 0) ? 1u : 0u;
        c1 += (i < n && g == 1) ? 1u : 0u;
    }
    c0 = wave_incl_sum<uint32_t>(c0), c1 = wave_incl_sum<uint32_t>(c1);
    const uint32_t n0 = (uint32_t)__shfl((int)c0, 63, 64), n1 = (uint32_t)__shfl((int)c1, 63, 64);
    const uint32_t n2 = n - n0 - n1;
    if (n0 > CAP || n1 > CAP || n2 > CAP) {  // uniform
        if (lane == 0) fb[atomicAdd(fb_count, 1u)] = q;
        return;
    }
    // 4. each range in order: its keys gathered into the (dead) table, read back 8 per lane, counted
    const int sh = 2 * k - src.F;
    const uint64_t klo = (uint64_t)b.c0 << sh, khi = ((uint64_t)b.c1 << sh) - 1ull;
    uint64_t pre = 0;
    for (uint32_t g = 0; g < P; ++g) {
        const uint32_t ng = g == 0 ? n0 : g == 1 ? n1 : n2;
        uint32_t at = 0;
    #pragma unroll
        for (int r = 0; r < R; ++r) {
            const uint32_t i = r * 64 + lane;
            const unsigned long long key = kr[r];  // gathered as staged (key and weight)
            const bool mine = i < n && range_of(key & ws.kmask) == g;
            const uint64_t m = __ballot(mine);
            if (mine)
                w.k[at + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))] = key;
            at += (uint32_t)__popcll(m);
        }
        wave_lds_sync();
        uint64_t kk[WKPT];
#pragma unroll
        for (int j = 0; j < WKPT; ++j) {
            const uint32_t i = j * 64 + lane;
            kk[j] = i < ng ? w.k[i] : EMPTY_KEY;
        }
        wave_lds_sync();  // read back before the count clears the table
        const uint64_t lo = g == 0 ? klo : (g == 1 ? sp0 : sp1) + 1ull;
        const uint64_t hi = g + 1 == P ? khi : (g == 0 ? sp0 : sp1);
        const int span = hi > lo ? 64 - __builtin_clzll(hi - lo) : 0;
        pre += wave_count_keys<CAP, SL, ORD>(w, b.begin + pre, ng, lo, span, 0, kk, ws, out_keys, out_counts, nullptr);
    }
    if (lane == 0) bucket_unique[q] = pre;
}

hipError_t launch_bucket_count64_parts(const BucketSrc &src, const Bucket *buckets, const uint32_t *list,
                                       uint64_t nlist, int k, uint64_t *out_keys, uint32_t *out_counts,
                                       uint64_t *bucket_unique, uint32_t *fb, unsigned int *fb_count, hipStream_t s,
                                       bool ordered) {
    if (!nlist) return hipSuccess;
#define FK_W64P(MS_, ORD_)                                                                                   \
    k_bucket_count64_parts<MS_, ORD_><<<(unsigned)nlist, 64, 0, s>>>(src, buckets, list, k, out_keys, out_counts, \
                                                                     bucket_unique, fb, fb_count)
    if (src.np > 0 && ordered)
        FK_W64P(true, true);
    else if (src.np > 0)
        FK_W64P(true, false);
    else if (ordered)
        FK_W64P(false, true);
    else
        FK_W64P(false, false);
#undef FK_W64P
    return hipGetLastError();
}
// The mid tier's buckets (513 .. 1024 keys) of a job whose keys repeat (configs[1]: ~10 copies of a
// k-mer; its 59 K mid buckets hold ~100 distinct keys each) straight on the wave tier's 512-key table:
// all 1024 keys loaded at once, inserted row by row; a bucket with more than 512 distinct keys gives
// up (nothing written) and is listed for the 1024-key kernel (fb / fb_count).  The 1024-key kernel's
// 14.8 KB of LDS held 2.7 waves per SIMD and ran last in the count (configs[1] tail,
// profiles/r06zh_c2_tail.txt).
template <bool MS, bool ORD>
__global__ __launch_bounds__(64) void k_bucket_count64_mid512(BucketSrc src, const Bucket *__restrict__ buckets,
                                                              const uint32_t *__restrict__ list, int k,
                                                              uint64_t *__restrict__ out_keys,
                                                              uint32_t *__restrict__ out_counts,
                                                              uint64_t *__restrict__ bucket_unique,
                                                              uint32_t *__restrict__ fb, unsigned int *fb_count) {
    constexpr uint32_t CAP = WAVE_BUCKET_CAP, SL = WAVE_SLOTS;
    constexpr int WKPT = WaveCfg<CAP>::KPT, R = 2 * WKPT;
    static_assert(R * 64 == WAVE_MID_CAP, "two rows of the wave tier's keys per lane cover the mid tier");
    __shared__ __attribute__((aligned(16))) WaveLds<CAP, SL> w;
    const uint32_t q = list[blockIdx.x];
    const Bucket b = buckets[q];
    PieceStarts ps{};
    if constexpr (MS)
        if (src.starts) ps = src.starts[q];
    uint64_t kk[R];
    wave_bucket_load<WAVE_MID_CAP, MS, R>(src, b, ps, true, kk, reinterpret_cast<const uint64_t *>(buckets));
    const int sh = 2 * k - src.F;
    const int span_bits = (32 - __builtin_clz(b.c1 - b.c0)) + sh;
    const uint32_t U = wave_count_keys<CAP, SL, ORD, WKPT, R>(w, b.begin, b.n, (uint64_t)b.c0 << sh, span_bits, q, kk,
                                                              wkey_spec(k, src.weighted), out_keys, out_counts,
                                                              bucket_unique);
    if (U == ~0u && (threadIdx.x & 63) == 0) fb[atomicAdd(fb_count, 1u)] = q;
}

hipError_t launch_bucket_count64_mid512(const BucketSrc &src, const Bucket *buckets, const uint32_t *list,
                                        uint64_t nlist, int k, uint64_t *out_keys, uint32_t *out_counts,
                                        uint64_t *bucket_unique, uint32_t *fb, unsigned int *fb_count, hipStream_t s,
                                        bool ordered) {
    if (!nlist) return hipSuccess;
#define FK_W64M5(MS_, ORD_)                                                                                    \
    k_bucket_count64_mid512<MS_, ORD_><<<(unsigned)nlist, 64, 0, s>>>(src, buckets, list, k, out_keys, out_counts, \
                                                                      bucket_unique, fb, fb_count)
    if (src.np > 0 && ordered)
        FK_W64M5(true, true);
    else if (src.np > 0)
        FK_W64M5(true, false);
    else if (ordered)
        FK_W64M5(false, true);
    else
        FK_W64M5(false, false);
#undef FK_W64M5
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// 5a''. heavy buckets split into wave-sized sub-buckets (k <= 32).  A bucket above the wave tier's
//      512 keys is (nearly always) one cell of its bin holding a minimizer-prefix cluster: a
//      canonical k-mer often starts with its own minimizer, so the cluster's keys share their
//      leading bits -- and the bits after the cell's as well, which is why a cut by the key bits
//      below the common prefix of the bucket's smallest and largest key left most clusters in one
//      sub-bucket (c3: 5.3 ms of split kernels for 1 ms off the block / big tiers).  The cut is by
//      splitters instead (a sample sort): 16 samples per sub-bucket of ~SPL_TGT keys, sorted in LDS,
//      every 16th a splitter; a key's sub-bucket = the splitters below it, so the sub-buckets are
//      ascending key ranges (their sorted outputs concatenate to the bucket's) and every copy of a
//      key lands in one sub-bucket.  The keys are copied in sub-bucket order (a counting sort in
//      LDS, k_bucket_split64), and counted in order by one wave per bucket (k_sub_count64_seq),
//      each sub-bucket's distinct keys straight after the previous ones' in the bucket's output (a
//      wave per two sub-buckets, then a kernel compacting their outputs, measured 1 ms slower at the
//      configs[2] load, profiles/r05x_sub_seq_ab.txt).  A bucket with a sub-bucket above 512 keys (a
//      k-mer repeated that often) keeps the block / big-table path.
// ---------------------------------------------------------------------------
constexpr uint32_t SPL_TGT = 256;  // target keys per sub-bucket (the wave tier takes up to 512)
constexpr uint32_t SPL_OVER = 16;     // samples per sub-bucket

// a split bucket's room in the split copy: slots = true (64-bit keys), a SPL_SLOT-key region per
// sub-bucket of the first cut (k_bucket_split64 scatters into them in its counting pass), and at least
// its keys (the second cut's contiguous copy); else its keys
constexpr uint32_t SPL_SLOT = WAVE_BUCKET_CAP;
__device__ __host__ inline uint64_t split_room(uint32_t n, bool slots) {
    if (!slots) return n;
    uint32_t ns = (n + SPL_TGT - 1) / SPL_TGT;
    ns = ns < 256u ? ns : 256u;  // WSPL_MAXS
    const uint64_t r = (uint64_t)ns * SPL_SLOT;
    return r > n ? r : n;
}
__global__ void k_listed_sizes(const Bucket *__restrict__ buckets, const uint32_t *__restrict__ list0, uint32_t n0,
                               const uint32_t *__restrict__ list1, uint32_t n1, uint64_t *__restrict__ sizes,
                               bool slots) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n0 + n1) return;
    sizes[i] = split_room(buckets[i < n0 ? list0[i] : list1[i - n0]].n, slots);
}

hipError_t launch_listed_sizes(const Bucket *buckets, const uint32_t *list0, uint32_t n0, const uint32_t *list1,
                               uint32_t n1, uint64_t *sizes, hipStream_t s, bool slots) {
    if (!(n0 + n1)) return hipSuccess;
    k_listed_sizes<<<(n0 + n1 + NT - 1) / NT, NT, 0, s>>>(buckets, list0, n0, list1, n1, sizes, slots);
    return hipGetLastError();
}

// One wave per listed bucket (no workgroup barrier: the workgroup version's ~40 barriers per bucket,
// through the sample sort, made it latency-bound at 3.3 ms for the configs[2] load's big tier).  At
// most WSPL_MAXS sub-buckets and WSPL_SMAX samples (9 KB of LDS per wave); a key's sub-bucket is
// searched again in the scatter pass.
constexpr uint32_t WSPL_MAXS = 256;
static_assert(WSPL_MAXS == 256, "split_room's sub-bucket cap");
constexpr uint32_t WSPL_SMAX = 1024;
constexpr int WSPL_PER = WSPL_MAXS / 64;  // sub-buckets per lane in the scans
constexpr int WSPL_KB = 8;                // keys per lane in flight in the counting and scatter passes

__global__ __launch_bounds__(64) void k_bucket_split64(BucketSrc src, const Bucket *__restrict__ buckets,
                                                       const uint32_t *__restrict__ list0, uint32_t n0,
                                                       const uint32_t *__restrict__ list1,
                                                       const uint64_t *__restrict__ sbase,
                                                       uint64_t *__restrict__ skeys, SubBucket *__restrict__ subs,
                                                       SplitParent *__restrict__ parents, unsigned int *counts,
                                                       uint32_t *__restrict__ fb0, uint32_t *__restrict__ fb1,
                                                       uint32_t block_cap, int sh, int retry, uint64_t kmask) {
    // kmask: the k-mer's bits of a staged key (WKeySpec) -- the sample and a key's sub-bucket go by the
    // k-mer alone, the staged word (key and weight) is passed through to the sub-bucket
    __shared__ uint64_t s_smp[WSPL_SMAX];  // the sample, sorted; then the splitters
    __shared__ uint32_t s_cnt[WSPL_MAXS];
    const uint32_t lane = threadIdx.x;
    const uint32_t i = blockIdx.x;
    const uint32_t q = i < n0 ? list0[i] : list1[i - n0];
    const Bucket b = buckets[q];
    const BucketView v = (src.np > 0 && src.starts) ? bucket_view_starts(src, src.starts[q]) : bucket_view(src, b);
    uint32_t ns0 = (b.n + SPL_TGT - 1) / SPL_TGT;
    ns0 = ns0 < WSPL_MAXS ? ns0 : WSPL_MAXS;
    // a sub-bucket above the wave's 512 keys is mostly the sample's bad luck (the keys between two
    // splitters 16 samples apart exceed twice their mean for ~4e-5 of the sub-buckets: ~40 buckets of
    // the configs[2] load, whose block / big-table fallback kernels then waited for LDS behind the wave
    // tier and ran after it, profiles/r06zh_side_prio_split_retry.txt): such a bucket is cut again into twice as many
    // sub-buckets from another sample; only a second oversized cut (a k-mer repeated that often) falls back
    uint32_t ns = ns0, nsp = 0, S = 64;
    const uint32_t c0 = lane * WSPL_PER;
    uint32_t cv[WSPL_PER], sum = 0, ne = 0, big = 0, isum = 0, ine = 0, netot = 0, bigmax = 0;
    auto sub_of = [&](uint64_t x) {  // the splitters below x (a lower bound over the nsp ascending ones)
        uint32_t lo = 0, len = nsp;
        while (len > 0) {
            const uint32_t half = len >> 1;
            if (s_smp[lo + half] < x) lo += half + 1, len -= half + 1;
            else len = half;
        }
        return lo;
    };
    const uint64_t *klast = bucket_key_ptr(v, b.n - 1);
    // the rows' piece bases 64 rows (4096 keys) at a time (row_bases; the passes below go in row order)
    RowBases rb{};
    uint32_t rb_first = ~0u;
    auto key_at = [&](uint32_t row0, uint32_t j) {
        const uint32_t row = row0 >> 6;
        if ((row & ~63u) != rb_first) {  // uniform
            rb_first = row & ~63u;
            rb = row_bases(v, rb_first);
        }
        const uint64_t *pa = row_key_ptr(v, rb, (int)(row & 63u), j);
        return ldg_nt<uint64_t>(j < b.n ? pa : klast);
    };
    const uint64_t sb = sbase[i];  // the bucket's room in the split copy (split_room)
    bool direct = false;           // uniform: the first cut's keys went straight into their sub-buckets' slots
    for (int att = 0; att < 2; ++att) {
        if (att) {  // uniform: the retry
            ns = 2 * ns0 < WSPL_MAXS ? 2 * ns0 : WSPL_MAXS;
            wave_lds_sync();  // the first cut's counts are read
        }
        S = 64;
        while (S < ns * SPL_OVER && S < WSPL_SMAX) S <<= 1;
        // 1. the sample (S keys spread over the bucket's copy order, which follows the reads, not the
        //    keys; the retry's half a stride later), bitonic-sorted in LDS by the wave
        const uint64_t soff = att ? (uint64_t)b.n / (2 * S) : 0;
        for (uint32_t j = lane; j < S; j += 64)
            s_smp[j] = *bucket_key_ptr(v, (uint32_t)(((uint64_t)j * b.n) / S + soff)) & kmask;
        for (uint32_t t = lane; t < WSPL_MAXS; t += 64) s_cnt[t] = 0;
        wave_lds_sync();
        for (uint32_t kk = 2; kk <= S; kk <<= 1) {
            for (uint32_t j = kk >> 1; j > 0; j >>= 1) {
                for (uint32_t t = lane; t < S / 2; t += 64) {
                    const uint32_t a = ((t & ~(j - 1)) << 1) | (t & (j - 1)), c = a + j;
                    const uint64_t x = s_smp[a], y = s_smp[c];
                    if ((x > y) == ((a & kk) == 0)) s_smp[a] = y, s_smp[c] = x;
                }
                wave_lds_sync();
            }
        }
        // 2. splitters: sample (t + 1) * S / ns - 1 for t < ns - 1, to the front (read, then written)
        nsp = ns - 1;
        uint64_t spv[WSPL_PER];
#pragma unroll
        for (int r = 0; r < WSPL_PER; ++r) {
            const uint32_t t = r * 64 + lane;
            if (t < nsp) spv[r] = s_smp[((uint64_t)(t + 1) * S) / ns - 1];
        }
        wave_lds_sync();
#pragma unroll
        for (int r = 0; r < WSPL_PER; ++r) {
            const uint32_t t = r * 64 + lane;
            if (t < nsp) s_smp[t] = spv[r];
        }
        wave_lds_sync();
        // 3. keys per sub-bucket (WSPL_KB keys per lane loaded before any is used: the loads overlap;
        //    every lane loads, past the bucket its last key, so that no load is branched over).  The
        //    first cut also stores each key into its sub-bucket's SPL_SLOT-key region of the bucket's
        //    room: no second pass (keys, searches, cursors) unless a sub-bucket overflows it
        for (uint32_t j0 = 0; j0 < b.n; j0 += 64 * WSPL_KB) {
            uint64_t x[WSPL_KB];
#pragma unroll
            for (int r = 0; r < WSPL_KB; ++r) x[r] = key_at(j0 + r * 64, j0 + r * 64 + lane);
#pragma unroll
            for (int r = 0; r < WSPL_KB; ++r)
                if (j0 + r * 64 + lane < b.n) {
                    const uint32_t sub = sub_of(x[r] & kmask);
                    const uint32_t at = atomicAdd(&s_cnt[sub], 1u);
                    if (att == 0 && at < SPL_SLOT) skeys[sb + (uint64_t)sub * SPL_SLOT + at] = x[r];
                }
        }
        wave_lds_sync();
        // 4. lane l's WSPL_PER consecutive sub-buckets: offsets (exclusive scan), non-empty ones, the largest
        sum = 0, ne = 0, big = 0;
#pragma unroll
        for (int t = 0; t < WSPL_PER; ++t) {
            cv[t] = s_cnt[c0 + t];  // zero past ns
            sum += cv[t];
            ne += cv[t] ? 1u : 0u;
            big = cv[t] > big ? cv[t] : big;
        }
        isum = wave_incl_sum<uint32_t>(sum), ine = wave_incl_sum<uint32_t>(ne);
        netot = (uint32_t)__shfl((int)ine, 63, 64);
        bigmax = (uint32_t)__shfl((int)wave_incl_max<uint32_t>(big), 63, 64);
        direct = att == 0;
        if ((bigmax <= WAVE_BUCKET_CAP && !(retry && att == 0)) || ns0 >= WSPL_MAXS) break;  // uniform
    }
    static_assert(SPL_SLOT >= WAVE_BUCKET_CAP, "a sub-bucket the wave tier takes fits its slot region");
    if (bigmax > WAVE_BUCKET_CAP) {  // uniform: a sub-bucket too large for a wave, the old path counts it
        if (lane == 0) {
            parents[i] = SplitParent{0u, 0u};
            if (b.n <= block_cap)
                fb0[atomicAdd(&counts[1], 1u)] = q;
            else
                fb1[atomicAdd(&counts[2], 1u)] = q;
        }
        return;
    }
    uint32_t first = 0;
    if (lane == 0) first = atomicAdd(&counts[0], netot);
    first = (uint32_t)__shfl((int)first, 0, 64);
    if (lane == 0) parents[i] = SplitParent{first, netot};
    // the bucket's key range: its cells [c0, c1) of the bin (c1 << sh wraps to 0 for the last cell of
    // 64-bit keys: its end - 1 is then ~0)
    const uint64_t klo = (uint64_t)b.c0 << sh, khi = ((uint64_t)b.c1 << sh) - 1ull;
    uint32_t off = isum - sum, nei = ine - ne;
#pragma unroll
    for (int t = 0; t < WSPL_PER; ++t) {
        const uint32_t sidx = c0 + t, c = cv[t];
        if (c) {
            // sub-bucket sidx holds keys in (splitter sidx - 1, splitter sidx]
            const uint64_t lo = sidx == 0 ? klo : s_smp[sidx - 1] + 1ull;
            const uint64_t hi = sidx == nsp ? khi : s_smp[sidx];
            SubBucket d;
            d.src = direct ? sb + (uint64_t)sidx * SPL_SLOT : sb + off;
            d.lo = lo;
            d.n = c;
            d.span = hi > lo ? 64u - (uint32_t)__builtin_clzll(hi - lo) : 0u;
            subs[first + nei] = d;
            ++nei;
        }
        s_cnt[sidx] = off;  // the sub-bucket's cursor
        off += c;
    }
    if (direct) return;  // uniform: the keys are in place
    wave_lds_sync();
    // 5. the second cut's keys in sub-bucket order, contiguous
    for (uint32_t j0 = 0; j0 < b.n; j0 += 64 * WSPL_KB) {
        uint64_t x[WSPL_KB];
#pragma unroll
        for (int r = 0; r < WSPL_KB; ++r) x[r] = key_at(j0 + r * 64, j0 + r * 64 + lane);
#pragma unroll
        for (int r = 0; r < WSPL_KB; ++r)
            if (j0 + r * 64 + lane < b.n) skeys[sb + atomicAdd(&s_cnt[sub_of(x[r] & kmask)], 1u)] = x[r];
    }
}

hipError_t launch_bucket_split64(const BucketSrc &src, const Bucket *buckets, const uint32_t *list0, uint32_t n0,
                                 const uint32_t *list1, uint32_t n1, const uint64_t *sbase, uint64_t *skeys,
                                 SubBucket *subs, SplitParent *parents, unsigned int *counts, uint32_t *fb0,
                                 uint32_t *fb1, uint32_t block_cap, int k, int F, hipStream_t s, bool retry) {
    if (!(n0 + n1)) return hipSuccess;
    k_bucket_split64<<<n0 + n1, 64, 0, s>>>(src, buckets, list0, n0, list1, sbase, skeys, subs, parents, counts, fb0,
                                            fb1, block_cap, 2 * k - F, retry ? 1 : 0, wkey_spec(k, src.weighted).kmask);
    return hipGetLastError();
}

// The wave tier over the split buckets' sub-buckets, one wave per split bucket, its sub-buckets in
// order: sub-bucket j's distinct keys go straight after those of sub-buckets 0 .. j - 1 at the
// bucket's output (ascending: the splitters cut the key range in order; useHT: table order per
// sub-bucket), so nothing is joined afterwards.  The next sub-bucket's keys are loaded while the
// current one is counted.  list[i] = the bucket of parents[i].
template <bool ORD>
__global__ __launch_bounds__(64) void k_sub_count64_seq(const Bucket *__restrict__ buckets,
                                                        const uint32_t *__restrict__ list,
                                                        const SplitParent *__restrict__ parents,
                                                        const SubBucket *__restrict__ subs,
                                                        const uint64_t *__restrict__ skeys, const WKeySpec ws,
                                                        uint64_t *__restrict__ out_keys,
                                                        uint32_t *__restrict__ out_counts,
                                                        uint64_t *__restrict__ bucket_unique) {
    constexpr uint32_t CAP = WAVE_BUCKET_CAP, SL = WAVE_SLOTS;
    constexpr int WKPT = WaveCfg<CAP>::KPT;
    __shared__ __attribute__((aligned(16))) WaveLds<CAP, SL> w;
    const SplitParent P = parents[blockIdx.x];
    if (P.nsub == 0) return;  // left to the block / big kernels
    const uint32_t q = list[blockIdx.x];
    const uint64_t begin = buckets[q].begin;
    const int lane = threadIdx.x & 63;
    // every lane loads (past the sub-bucket: its first key), so the next sub-bucket's loads are never
    // branched over and the count of this one waits for its own keys only
    auto load = [&](const SubBucket &d, uint64_t (&kk)[WKPT]) {
#pragma unroll
        for (int jj = 0; jj < WKPT; ++jj) {
            const uint32_t i = jj * 64 + lane;
            const bool ok = i < d.n;
            const uint64_t x = ldg_nt<uint64_t>(&skeys[d.src + (ok ? i : 0u)]);
            kk[jj] = ok ? x : EMPTY_KEY;
        }
    };
    SubBucket d0 = subs[P.first], d1;
    uint64_t ka[WKPT], kb[WKPT];
    load(d0, ka);
    uint64_t pre = 0;
    for (uint32_t j = 0;; ++j) {
        const bool more = j + 1 < P.nsub;
        d1 = subs[P.first + (more ? j + 1 : j)];  // the last round reloads its own (unused)
        load(d1, kb);
        pre += wave_count_keys<CAP, SL, ORD>(w, begin + pre, d0.n, d0.lo, (int)d0.span, 0, ka, ws, out_keys,
                                             out_counts, nullptr);
        if (!more) break;
        d0 = d1;  // one call site: the prefetched keys move over
#pragma unroll
        for (int jj = 0; jj < WKPT; ++jj) ka[jj] = kb[jj];
    }
    if (lane == 0) bucket_unique[q] = pre;
}

hipError_t launch_sub_count64_seq(const Bucket *buckets, const uint32_t *list, uint32_t nl, const SplitParent *parents,
                                  const SubBucket *subs, const uint64_t *skeys, int k, bool weighted,
                                  uint64_t *out_keys, uint32_t *out_counts, uint64_t *bucket_unique, hipStream_t s,
                                  bool ordered) {
    if (!nl) return hipSuccess;
    const WKeySpec ws = wkey_spec(k, weighted);
    if (ordered)
        k_sub_count64_seq<true><<<nl, 64, 0, s>>>(buckets, list, parents, subs, skeys, ws, out_keys, out_counts,
                                                  bucket_unique);
    else
        k_sub_count64_seq<false><<<nl, 64, 0, s>>>(buckets, list, parents, subs, skeys, ws, out_keys, out_counts,
                                                   bucket_unique);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// 5a''. wave tier for 128-bit keys (33 <= k <= 63): the same one-wave count
//      with keys held as (hi, lo) words.  A slot is claimed by a
//      compare-and-swap on its hi word (hi < 2^62 for k <= 63, so ~0 marks an
//      empty slot); the claimer then stores lo, and a key whose hi matches
//      compares lo only after a wave-local LDS wait, so it sees that store.
//      Each round of the probe loop is wave-uniform (claim, store, wait,
//      compare), which keeps that order however the lanes diverge.
// ---------------------------------------------------------------------------

constexpr uint32_t W2CAP = WAVE128_BUCKET_CAP;

// CAP keys per bucket (W2CAP, or WAVE128_MID_CAP for the listed mid tier), SL slots (2 * CAP, or
// 3 / 2 * CAP as the 64-bit tier); the distinct keys' group-ordered copy is written over the dead
// table, the group counts and cursors in its hi words above CAP
template <uint32_t CAP, uint32_t SL>
struct WaveLds128 {
    static_assert(SL >= CAP && SL % 8 == 0, "the table holds every distinct key; cleared 8 counts at a time");
    static_assert((SL - CAP) * 8 >= (CAP > 256 ? 2048u : 1024u), "group arrays above CAP");
    unsigned long long hi[SL], lo[SL];
    uint16_t c[SL];
    uint16_t list[CAP];
};

template <uint32_t SL>
__device__ __forceinline__ uint32_t wslot128(uint64_t hi, uint64_t lo) {
    const uint32_t h = (uint32_t)(((lo ^ (hi * 0xc2b2ae3d27d4eb4full)) * 0x9e3779b97f4a7c15ull) >> 32);
    return (uint32_t)(((uint64_t)h * SL) >> 32);
}

// 3. the rank of U distinct 128-bit keys (key i = j * 64 + lane in th / tl, counts tc) inside G groups
//    of the key range [lo_b, lo_b + 2^span_bits): G = 64, 128 when more than 64 distinct keys, 256 above
//    128 (CAP 512); each key with its count written at out_keys / out_counts + begin + its rank.  LDS:
//    g_hi / g_lo / g_c hold the group-ordered copy (>= U entries, dead before the call), s_gcnt the
//    group counts and cursors (2 x 128 words, 2 x 256 for CAP 512), s_scnt 128 words.
// one 128-bit key (hi, lo words) at pair index i of out: one 16-B store
__device__ __forceinline__ void store_key128(uint64_t *out, uint64_t i, uint64_t hi, uint64_t lo) {
    typedef uint64_t u64x2s __attribute__((ext_vector_type(2)));
    u64x2s v;
    v.x = hi;
    v.y = lo;
    reinterpret_cast<u64x2s *>(out)[i] = v;
}

template <uint32_t CAP, int W2KPT>
__device__ __forceinline__ void wave_rank128(unsigned long long *g_hi, unsigned long long *g_lo, uint16_t *g_c,
                                             uint32_t *s_gcnt, uint32_t *s_scnt, uint32_t U, const uint64_t (&th)[W2KPT],
                                             const uint64_t (&tl)[W2KPT], const uint16_t (&tc)[W2KPT], u128 lo_b,
                                             int span_bits, uint64_t begin, uint64_t *__restrict__ out_keys,
                                             uint32_t *__restrict__ out_counts) {
    const int lane = threadIdx.x & 63;
    const int gw = (CAP > 256 && U > 128) ? 2 : (U > 64 ? 1 : 0);  // uniform: 256 / 128 / 64 groups
    const int gbits = 6 + gw;
    const int gsh = span_bits > gbits ? span_bits - gbits : 0;
    // (key - lo_b) >> gsh from 64-bit words: the group bits lie in the high word of the difference
    // whenever gsh >= 64 (k = 55: gsh ~ 90), a funnel of both words below (a uniform branch)
    const uint64_t lbh = (uint64_t)(lo_b >> 64), lbl = (uint64_t)lo_b;
    auto group = [&](uint64_t h, uint64_t l) -> uint32_t {
        const uint64_t dh = h - lbh - (l < lbl ? 1ull : 0ull);
        if (gsh >= 64) return (uint32_t)(dh >> (gsh - 64));
        if (gsh == 0) return (uint32_t)(l - lbl);
        return (uint32_t)((dh << (64 - gsh)) | ((l - lbl) >> gsh));
    };
    uint32_t *s_gcur = s_gcnt + (CAP > 256 ? 256 : 128);
    wave_lds_sync();  // the table reads above are done before the table is overwritten below
    if (gw == 2)
        reinterpret_cast<uint4 *>(s_gcnt)[lane] = make_uint4(0, 0, 0, 0);
    else if (gw == 1)
        reinterpret_cast<uint2 *>(s_gcnt)[lane] = make_uint2(0, 0);
    else
        s_gcnt[lane] = 0;
    wave_lds_sync();
#pragma unroll
    for (int j = 0; j < W2KPT; ++j)
        if (j * 64 + lane < (int)U) atomicAdd(&s_gcnt[group(th[j], tl[j])], 1u);
    wave_lds_sync();
    if (gw == 2) {  // lane l owns groups 4l .. 4l + 3
        const uint4 c = reinterpret_cast<const uint4 *>(s_gcnt)[lane];
        const uint32_t t = c.x + c.y + c.z + c.w;
        const uint32_t base = wave_incl_sum<uint32_t>(t) - t;
        reinterpret_cast<uint4 *>(s_gcur)[lane] = make_uint4(base, base + c.x, base + c.x + c.y, base + c.x + c.y + c.z);
    } else if (gw == 1) {  // lane l owns groups 2l, 2l + 1
        const uint2 c = reinterpret_cast<const uint2 *>(s_gcnt)[lane];
        const uint32_t t = c.x + c.y;
        const uint32_t base = wave_incl_sum<uint32_t>(t) - t;
        reinterpret_cast<uint2 *>(s_gcur)[lane] = make_uint2(base, base + c.x);
    } else {
        const uint32_t gc = s_gcnt[lane];
        s_gcur[lane] = wave_incl_sum<uint32_t>(gc) - gc;
    }
    wave_lds_sync();
#pragma unroll
    for (int j = 0; j < W2KPT; ++j) {
        if (j * 64 + lane < (int)U) {
            const uint32_t p = atomicAdd(&s_gcur[group(th[j], tl[j])], 1u);
            g_hi[p] = th[j];
            g_lo[p] = tl[j];
            g_c[p] = tc[j];
        }
    }
    wave_lds_sync();
    // 3b. groups of more than RANK_BIG128 keys (a minimizer-prefix cluster: k-mers of the bin that start
    //     with the same minimizer share its 2m bits below the cell's, so they fall into one group and
    //     each of their keys' rank loops would run over the whole cluster) are ranked by a second cut,
    //     as in the 64-bit tier: 64 sub-groups by the 6 bits below the group's own common prefix (from
    //     the OR of its keys' XOR with its first), counted, scattered in place, then the rank loop over
    //     a key's sub-group.  One group at a time, the wave's lanes over its keys.
    constexpr uint32_t RANK_BIG128 = 24;
    static_assert(CAP >= 256, "64 + 64 sub-group counters");
    uint32_t *s_scur = s_scnt + 64;
    const int ncomp = 1 << gw;  // groups per lane: lane l owns groups l * ncomp .. + ncomp - 1
    for (int comp = 0; comp < ncomp; ++comp) {
        const uint32_t mine = s_gcnt[lane * ncomp + comp];
        uint64_t bm = __ballot(mine > RANK_BIG128);
        while (bm) {  // uniform
            const uint32_t g = (uint32_t)(__builtin_ctzll(bm) * ncomp + comp);
            bm &= bm - 1;
            const uint32_t cnt = s_gcnt[g], g0 = s_gcur[g] - cnt;
            const uint64_t xh = g_hi[g0], xl = g_lo[g0];
            uint64_t gh[W2KPT], gl[W2KPT];
            uint16_t gc[W2KPT];
            uint64_t oh = 0, ol = 0;
#pragma unroll
            for (int j = 0; j < W2KPT; ++j) {
                const uint32_t i = j * 64 + lane;
                if (i < cnt) {
                    gh[j] = g_hi[g0 + i];
                    gl[j] = g_lo[g0 + i];
                    gc[j] = g_c[g0 + i];
                    oh |= gh[j] ^ xh;
                    ol |= gl[j] ^ xl;
                }
            }
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) {
                oh |= (uint64_t)__shfl_xor((long long)oh, d, 64);
                ol |= (uint64_t)__shfl_xor((long long)ol, d, 64);
            }
            // the group's keys agree above bit hb of the 128-bit key
            const int hb = oh ? 127 - __builtin_clzll(oh) : 63 - __builtin_clzll(ol | 1ull);
            const int ssh = hb >= 5 ? hb - 5 : 0;
            auto sub = [&](uint64_t h, uint64_t l) { return (uint32_t)((((u128)h << 64) | l) >> ssh) & 63u; };
            s_scnt[lane] = 0;
            wave_lds_sync();
#pragma unroll
            for (int j = 0; j < W2KPT; ++j)
                if (j * 64 + lane < (int)cnt) atomicAdd(&s_scnt[sub(gh[j], gl[j])], 1u);
            wave_lds_sync();
            const uint32_t sc = s_scnt[lane];
            s_scur[lane] = wave_incl_sum<uint32_t>(sc) - sc;
            wave_lds_sync();
#pragma unroll
            for (int j = 0; j < W2KPT; ++j) {
                if (j * 64 + lane < (int)cnt) {
                    const uint32_t p = g0 + atomicAdd(&s_scur[sub(gh[j], gl[j])], 1u);
                    g_hi[p] = gh[j];
                    g_lo[p] = gl[j];
                    g_c[p] = gc[j];
                }
            }
            wave_lds_sync();
#pragma unroll
            for (int j = 0; j < W2KPT; ++j) {
                if (j * 64 + lane < (int)cnt) {
                    const uint32_t sb = sub(gh[j], gl[j]);
                    const uint32_t s1 = g0 + s_scur[sb], s0 = s1 - s_scnt[sb];
                    uint32_t r = s0;
                    for (uint32_t t = s0; t < s1; ++t) {  // both words read, no branch per member
                        const uint64_t ht = g_hi[t], lt = g_lo[t];
                        r += (uint32_t)((ht < gh[j]) | ((ht == gh[j]) & (lt < gl[j])));
                    }
                    store_key128(out_keys, begin + r, gh[j], gl[j]);
                    out_counts[begin + r] = gc[j];
                }
            }
            wave_lds_sync();  // the sub-group counters are reused by the next group
        }
    }
    for (uint32_t p = lane; p < U; p += 64) {
        const uint64_t h = g_hi[p], l = g_lo[p];
        const uint32_t g = group(h, l);
        if (s_gcnt[g] > RANK_BIG128) continue;  // ranked above
        const uint32_t g1 = s_gcur[g], g0 = g1 - s_gcnt[g];  // the cursor ends at the group's end
        uint32_t r = g0;
        for (uint32_t j = g0; j < g1; j += 2) {  // two members per round, both words read, no branches
            const uint64_t h0 = g_hi[j], l0 = g_lo[j], h1 = g_hi[j + 1], l1 = g_lo[j + 1];
            r += (uint32_t)((h0 < h) | ((h0 == h) & (l0 < l))) +
                 (uint32_t)((j + 1 < g1) & ((h1 < h) | ((h1 == h) & (l1 < l))));
        }
        store_key128(out_keys, begin + r, h, l);
        out_counts[begin + r] = g_c[p];
    }
}

// count n <= CAP 128-bit keys (held in khi / klo) with the calling wave, as wave_count_keys: the distinct
// keys (hi, lo word pairs) with their counts at out_keys / out_counts + begin, ascending (ORD) or in table
// order (useHT), their number in uniq[q] (uniq may be null).  Every key lies in [lo_b, lo_b + 2^span_bits)
// (the rank's group cut).  Returns the number of distinct keys (wave-uniform).
template <uint32_t CAP, uint32_t SL, bool ORD = true, int W2KPT = CAP / 64>
__device__ __forceinline__ uint32_t wave_count_keys128(WaveLds128<CAP, SL> &w, uint64_t begin, uint32_t n, u128 lo_b,
                                                   int span_bits, uint64_t q, const uint64_t (&khi)[W2KPT],
                                                   const uint64_t (&klo)[W2KPT], uint64_t *__restrict__ out_keys,
                                                   uint32_t *__restrict__ out_counts,
                                                   uint64_t *__restrict__ uniq) {
    const int lane = threadIdx.x & 63;
    if (n == 0) {
        if (lane == 0 && uniq) uniq[q] = 0;
        return 0;
    }
    {
        ulonglong2 *h2 = reinterpret_cast<ulonglong2 *>(w.hi);
#pragma unroll
        for (uint32_t s = lane; s < SL / 2; s += 64) h2[s] = make_ulonglong2(EMPTY_KEY, EMPTY_KEY);
        uint4 *c4 = reinterpret_cast<uint4 *>(w.c);
#pragma unroll
        for (uint32_t s = lane; s < SL / 8; s += 64) c4[s] = make_uint4(0, 0, 0, 0);
    }
    wave_lds_sync();
    // 1. dedupe
    uint32_t sl[W2KPT];
    unsigned long long old[W2KPT];
#pragma unroll
    for (int j = 0; j < W2KPT; ++j) sl[j] = wslot128<SL>(khi[j], klo[j]);
#pragma unroll
    for (int j = 0; j < W2KPT; ++j) old[j] = w.hi[sl[j]];
    uint32_t U = 0;
#pragma unroll
    for (int j = 0; j < W2KPT; ++j) {
        const uint64_t hi = khi[j], lo = klo[j];
        bool done = hi == EMPTY_KEY, fresh = false;
        uint32_t s = sl[j];
        unsigned long long cur = old[j];
        while (__ballot(!done)) {
            const bool claim = !done && cur == EMPTY_KEY;
            if (claim) {
                cur = atomicCAS(&w.hi[s], EMPTY_KEY, (unsigned long long)hi);
                fresh = cur == EMPTY_KEY;
            }
            if (claim && fresh) w.lo[s] = lo;
            wave_lds_sync();
            if (!done) {
                if (fresh || (cur == hi && w.lo[s] == lo)) {
                    done = true;
                } else {
                    s = s + 1 == SL ? 0u : s + 1;
                    cur = w.hi[s];
                }
            }
        }
        if (hi != EMPTY_KEY) {
            atomicAdd(reinterpret_cast<uint32_t *>(&w.c[s & ~1u]), 1u << (16 * (s & 1u)));
            sl[j] = s;
        }
        const uint64_t m = __ballot(fresh);
        if (fresh)
            w.list[U + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))] =
                (uint16_t)s;
        U += (uint32_t)__popcll(m);
    }
    wave_lds_sync();
#if defined(FK_W64_STOP) && FK_W64_STOP == 1  // phase probe (measurement builds only): stop after the dedupe
    if (lane == 0 && uniq) uniq[q] = U;
    return U;
#endif
    // 2. the distinct keys and their counts into registers through the slot list (key i = j * 64 +
    //    lane); the table is dead after these reads
    uint64_t th[W2KPT], tl[W2KPT];
    uint16_t tc[W2KPT];
#pragma unroll
    for (int j = 0; j < W2KPT; ++j) {
        const uint32_t i = j * 64 + lane;
        if (i < U) {
            const uint32_t s = w.list[i];
            th[j] = w.hi[s];
            tl[j] = w.lo[s];
            tc[j] = w.c[s];
        }
    }
    if constexpr (!ORD) {  // useHT: the table's order, no rank (wave_count_keys)
#pragma unroll
        for (int j = 0; j < W2KPT; ++j) {
            const uint32_t i = j * 64 + lane;
            if (i < U) {
                store_key128(out_keys, begin + i, th[j], tl[j]);
                out_counts[begin + i] = tc[j];
            }
        }
        if (lane == 0 && uniq) uniq[q] = U;
        wave_lds_sync();
        return U;
    }
    // 3. rank (the group counts and cursors in the dead table's hi words above CAP, the group-ordered
    //    copy over the table, the second cut's counters in the dead slot list)
    wave_rank128<CAP, W2KPT>(w.hi, w.lo, w.c, reinterpret_cast<uint32_t *>(&w.hi[CAP]),
                             reinterpret_cast<uint32_t *>(w.list), U, th, tl, tc, lo_b, span_bits, begin, out_keys,
                             out_counts);
    if (lane == 0 && uniq) uniq[q] = U;
    wave_lds_sync();
    return U;
}

// ---- the main 128-bit wave tier, with a fingerprint table.  The uniform-round
// dedupe above waits on every probe round twice (the hi-word claim, then the lo word of a matching
// slot).  Here the table holds a 64-bit fingerprint of each key: a probe is one compare-and-swap or
// read per round, lanes probe independently (the 64-bit tier's loop), and with 2 * CAP slots the table
// is at most half full.  Then the claimers store their keys in claim order over the dead table, and
// every key is checked against its slot's claimer (a fingerprint shared by two different keys is
// caught there, and the bucket is counted exactly from the registers, wave_count_exact128).  The table
// takes 16 B per key of CAP like the uniform-round one's, with the counts in 32-bit words.
template <uint32_t CAP>
struct WaveLdsFp {
    static constexpr uint32_t SL = 2 * CAP;
    unsigned long long f[SL];  // fingerprints; then the distinct keys in claim order (hi words in
                               // [0, CAP), lo words in [CAP, 2 CAP)); then the rank's group-ordered copy
    uint32_t c[SL];            // per slot: count | claim index << 16; then the rank's counters
    uint16_t kc[CAP];          // the distinct keys' counts in claim order; then the group-ordered counts
};

// test hook (fk_debug_fingerprint_bits): the fingerprints cut to their low bits, so that distinct keys
// share fingerprints and the exact path runs; ~0 = whole fingerprints (the product)
__device__ uint64_t g_fp_mask = ~0ull;

__device__ __forceinline__ uint64_t fp128(uint64_t hi, uint64_t lo, uint64_t mask) {
    // for one hi word a bijection of lo (keys sharing hi never collide); ~0 is the empty slot
    const uint64_t f = (lo ^ ((hi + 0x9e3779b97f4a7c15ull) * 0xbf58476d1ce4e5b9ull)) & mask;
    return f == EMPTY_KEY ? f - 1 : f;
}

hipError_t set_fingerprint_bits(int bits) {
    const uint64_t m = bits >= 64 || bits <= 0 ? ~0ull : ((1ull << bits) - 1ull);
    return hipMemcpyToSymbol(HIP_SYMBOL(g_fp_mask), &m, sizeof m, 0, hipMemcpyHostToDevice);
}

// The exact count of n 128-bit keys held in LDS (s_hi / s_lo[0, n)), as wave_count_exact64: the rare
// path of a shared fingerprint (~U^2 / 2^65 per bucket).
__device__ __forceinline__ uint32_t wave_count_exact128(const unsigned long long *s_hi, const unsigned long long *s_lo,
                                                        uint16_t *s_cnt, uint32_t n, uint64_t begin,
                                                        uint64_t *__restrict__ out_keys,
                                                        uint32_t *__restrict__ out_counts) {
    const uint32_t lane = threadIdx.x & 63;
    for (uint32_t i = lane; i < n; i += 64) {
        const unsigned long long xh = s_hi[i], xl = s_lo[i];
        uint32_t cnt = 0;
        bool first = true;
        for (uint32_t t = 0; t < n; ++t) {
            const bool eq = s_hi[t] == xh && s_lo[t] == xl;
            cnt += eq ? 1u : 0u;
            first = first && !(eq && t < i);
        }
        s_cnt[i] = first ? (uint16_t)cnt : (uint16_t)0;
    }
    wave_lds_sync();
    uint32_t u = 0;
    for (uint32_t i = lane; i < n; i += 64) {
        const uint32_t c = s_cnt[i];
        if (!c) continue;
        const unsigned long long xh = s_hi[i], xl = s_lo[i];
        uint32_t r = 0;
        for (uint32_t t = 0; t < n; ++t) {
            const unsigned long long th = s_hi[t];
            r += (s_cnt[t] && (th < xh || (th == xh && s_lo[t] < xl))) ? 1u : 0u;
        }
        store_key128(out_keys, begin + r, xh, xl);
        out_counts[begin + r] = c;
        ++u;
    }
    return (uint32_t)__shfl((int)wave_incl_sum<uint32_t>(u), 63, 64);
}

template <uint32_t CAP, bool ORD = true, int W2KPT = CAP / 64>
__device__ __forceinline__ uint32_t wave_count_keys128_fp(WaveLdsFp<CAP> &w, uint64_t begin, uint32_t n, u128 lo_b,
                                                      int span_bits, uint64_t q, const uint64_t (&khi)[W2KPT],
                                                      const uint64_t (&klo)[W2KPT], uint64_t *__restrict__ out_keys,
                                                      uint32_t *__restrict__ out_counts,
                                                      uint64_t *__restrict__ uniq, uint64_t fpm) {
    constexpr uint32_t SL = WaveLdsFp<CAP>::SL;
    const int lane = threadIdx.x & 63;
    if (n == 0) {
        if (lane == 0 && uniq) uniq[q] = 0;
        return 0;
    }
    {
        ulonglong2 *f2 = reinterpret_cast<ulonglong2 *>(w.f);
#pragma unroll
        for (uint32_t s = lane; s < SL / 2; s += 64) f2[s] = make_ulonglong2(EMPTY_KEY, EMPTY_KEY);
        uint4 *c4 = reinterpret_cast<uint4 *>(w.c);
#pragma unroll
        for (uint32_t s = lane; s < SL / 4; s += 64) c4[s] = make_uint4(0, 0, 0, 0);
    }
    wave_lds_sync();
    // 1. dedupe on fingerprints, with the 64-bit tier's per-lane loop
    uint64_t fp[W2KPT];
    uint32_t sl[W2KPT], cidx[W2KPT];
#pragma unroll
    for (int j = 0; j < W2KPT; ++j) {
        fp[j] = khi[j] == EMPTY_KEY ? EMPTY_KEY : fp128(khi[j], klo[j], fpm);
        sl[j] = wslot<SL>(fp[j]);
    }
    static_assert((SL & (SL - 1)) == 0, "probe wrap by mask");
    uint32_t U = 0;
#pragma unroll
    for (int j = 0; j < W2KPT; ++j) {
        const uint64_t key = fp[j];
        bool fresh = false;
        uint32_t s = sl[j];
        if (key != EMPTY_KEY) {
            // every probe a compare-and-swap: an occupied slot returns its fingerprint, so a fresh key
            // takes one LDS round trip at its home slot instead of a read and then the swap (most keys
            // of a 128-bit bucket are distinct); 29.0 against 30.5 ms per configs[3]-load launch
            for (;;) {
                const unsigned long long prev = atomicCAS(&w.f[s], EMPTY_KEY, (unsigned long long)key);
                fresh = prev == EMPTY_KEY;
                if (fresh || prev == key) break;
                s = (s + 1) & (SL - 1);
            }
            sl[j] = s;
        }
        const uint64_t m = __ballot(fresh);
        const uint32_t idx = U + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        if (key != EMPTY_KEY) atomicAdd(&w.c[s], fresh ? 1u + (idx << 16) : 1u);
        cidx[j] = fresh ? idx : ~0u;
        U += (uint32_t)__popcll(m);
    }
    wave_lds_sync();
#if defined(FK_W128_STOP) && FK_W128_STOP == 1  // phase probe (measurement builds only): stop after the dedupe
    if (lane == 0 && uniq) uniq[q] = U;
    return U;
#endif
    // 2. the claimers' keys in claim order over the dead table; every key checked against its slot's
    //    claimer; the claimers' counts
    unsigned long long *kh = w.f, *kl = w.f + CAP;
#pragma unroll
    for (int j = 0; j < W2KPT; ++j)
        if (cidx[j] != ~0u) kh[cidx[j]] = khi[j], kl[cidx[j]] = klo[j];
    wave_lds_sync();
    bool bad = false;
#pragma unroll
    for (int j = 0; j < W2KPT; ++j) {
        if (fp[j] == EMPTY_KEY) continue;
        const uint32_t v = w.c[sl[j]], idx = v >> 16;
        bad |= kh[idx] != khi[j] || kl[idx] != klo[j];
        if (cidx[j] != ~0u) w.kc[idx] = (uint16_t)(v & 0xffffu);
    }
    if (__ballot(bad)) {  // uniform: two keys share a fingerprint -- the exact count of the n keys
        wave_lds_sync();
#pragma unroll
        for (int j = 0; j < W2KPT; ++j)
            if (j * 64 + lane < (int)n) kh[j * 64 + lane] = khi[j], kl[j * 64 + lane] = klo[j];
        wave_lds_sync();
        const uint32_t u = wave_count_exact128(kh, kl, w.kc, n, begin, out_keys, out_counts);
        if (lane == 0 && uniq) uniq[q] = u;
        wave_lds_sync();
        return u;
    }
    wave_lds_sync();
#if defined(FK_W128_STOP) && FK_W128_STOP == 2  // phase probe: stop after the claimers' check
    if (lane == 0 && uniq) uniq[q] = U;
    return U;
#endif
    uint64_t th[W2KPT], tl[W2KPT];
    uint16_t tc[W2KPT];
#pragma unroll
    for (int j = 0; j < W2KPT; ++j) {
        const uint32_t i = j * 64 + lane;
        if (i < U) th[j] = kh[i], tl[j] = kl[i], tc[j] = w.kc[i];
    }
    if constexpr (!ORD) {  // useHT: claim order, no rank
#pragma unroll
        for (int j = 0; j < W2KPT; ++j) {
            const uint32_t i = j * 64 + lane;
            if (i < U) {
                store_key128(out_keys, begin + i, th[j], tl[j]);
                out_counts[begin + i] = tc[j];
            }
        }
        if (lane == 0 && uniq) uniq[q] = U;
        wave_lds_sync();
        return U;
    }
    // 3. rank: the group-ordered copy over the claim-order arrays, the counters in the dead slot words
    constexpr uint32_t NG = CAP > 256 ? 256 : 128;
    static_assert(2 * NG + 128 <= SL, "group and sub-group counters in the slot words");
    wave_rank128<CAP, W2KPT>(kh, kl, w.kc, w.c, w.c + 2 * NG, U, th, tl, tc, lo_b, span_bits, begin, out_keys,
                             out_counts);
    if (lane == 0 && uniq) uniq[q] = U;
    wave_lds_sync();
    return U;
}

// one bucket (cells [c0, c1) of its bin) of <= CAP 128-bit keys with the calling wave
template <uint32_t CAP, uint32_t SL, bool ORD = true, int W2KPT = CAP / 64>
__device__ __forceinline__ void wave_count_bucket128(WaveLds128<CAP, SL> &w, const Bucket &b, uint64_t q,
                                                     const uint64_t (&khi)[W2KPT], const uint64_t (&klo)[W2KPT],
                                                     int k, int F, uint64_t *__restrict__ out_keys,
                                                     uint32_t *__restrict__ out_counts,
                                                     uint64_t *__restrict__ bucket_unique) {
    const int sh = 2 * k - F;
    const int span_bits = b.n ? (32 - __builtin_clz(b.c1 - b.c0)) + sh : 0;
    wave_count_keys128<CAP, SL, ORD, W2KPT>(w, b.begin, b.n, (u128)b.c0 << sh, span_bits, q, khi, klo, out_keys,
                                            out_counts, bucket_unique);
}

// list: bucket indices (the mid tier: buckets of CAP / 2 < n <= CAP keys), or null for every bucket
template <int BPW, uint32_t SL, bool MS = false, uint32_t CAP = W2CAP, bool ORD = true, bool FP = false>
__global__ __launch_bounds__(64) void k_bucket_count128_wave(BucketSrc src,
                                                             const Bucket *__restrict__ buckets, uint64_t nbuckets,
                                                             int k, uint64_t *__restrict__ out_keys,
                                                             uint32_t *__restrict__ out_counts,
                                                             uint64_t *__restrict__ bucket_unique,
                                                             const uint32_t *__restrict__ list = nullptr) {
    typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));
    constexpr int W2KPT = CAP / 64;
    using Lds = typename std::conditional<FP, WaveLdsFp<CAP>, WaveLds128<CAP, SL>>::type;
    __shared__ __attribute__((aligned(16))) Lds w;
    const uint64_t q0 = (uint64_t)blockIdx.x * BPW;
    const uint64_t fpm = FP ? g_fp_mask : 0ull;  // read once, not per bucket
    Bucket b[BPW];
    bool mine[BPW];
    uint64_t qq[BPW];
    uint64_t khi[BPW][W2KPT], klo[BPW][W2KPT];
    const uint64_t *dummy = reinterpret_cast<const uint64_t *>(buckets);
    // every lane loads (lanes past the bucket from `dummy`, a readable address): loads that are not
    // branched over let bucket 0's count wait for its own keys only (vmcnt(4), not 0)
    auto keys_load = [&](int t, const PieceStarts &ps) {
        BucketView bv{};
        RowBases rb{};
        if constexpr (MS) {
            if (mine[t]) {  // uniform
                bv = src.starts ? bucket_view_starts<2>(src, ps) : bucket_view<2>(src, b[t]);
                rb = row_bases<2>(bv);
            }
        }
#pragma unroll
        for (int j = 0; j < W2KPT; ++j) {
            const uint32_t i = j * 64 + (threadIdx.x & 63);
            const bool ok = mine[t] && i < b[t].n;
            const uint64_t *pa = MS ? row_key_ptr<2>(bv, rb, j, i) : src.keys + 2 * (b[t].begin + i);
            const uint64_t *a = ok ? pa : dummy;  // no branch on `ok`
            const u64x2 v = ldg_nt<u64x2>(a);
            khi[t][j] = ok ? v.x : EMPTY_KEY;
            klo[t][j] = ok ? v.y : EMPTY_KEY;
        }
    };
#pragma unroll
    for (int t = 0; t < BPW; ++t) {
        const uint64_t i = q0 + t;
        const uint64_t q = i < nbuckets ? (list ? (uint64_t)list[i] : i) : 0;
        qq[t] = q;
        // the piece starts are read beside the bucket (not after its size): one round trip before
        // the key loads instead of two
        PieceStarts ps{};
        if (i < nbuckets) {
            b[t] = buckets[q];
            if (MS && src.starts) ps = src.starts[q];
        }
        mine[t] = i < nbuckets && b[t].n <= CAP && (!list || b[t].n > CAP / 2);
        keys_load(t, ps);
    }
#pragma unroll
    for (int t = 0; t < BPW; ++t) {
        if (!mine[t]) continue;
#if defined(FK_W128_STOP) && FK_W128_STOP == 0  // phase probe: the key loads only
        if constexpr (FP) {
            uint64_t x = 0;
#pragma unroll
            for (int j = 0; j < W2KPT; ++j) x ^= khi[t][j] ^ klo[t][j];
            if ((threadIdx.x & 63) == 0 && bucket_unique) bucket_unique[qq[t]] = 0;
            if (x == 0x0123456789abcdefull) out_counts[0] = 1u;  // keeps the loads
            continue;
        }
#endif
        if constexpr (FP) {
            const int sh = 2 * k - src.F;
            const int span_bits = b[t].n ? (32 - __builtin_clz(b[t].c1 - b[t].c0)) + sh : 0;
            wave_count_keys128_fp<CAP, ORD>(w, b[t].begin, b[t].n, (u128)b[t].c0 << sh, span_bits, qq[t], khi[t],
                                            klo[t], out_keys, out_counts, bucket_unique, fpm);
        } else {
            wave_count_bucket128<CAP, SL, ORD>(w, b[t], qq[t], khi[t], klo[t], k, src.F, out_keys, out_counts,
                                               bucket_unique);
        }
    }
}

hipError_t launch_bucket_count128_wave_mid(const BucketSrc &src, const Bucket *buckets, const uint32_t *list,
                                           uint64_t nlist, int k, uint64_t *out_keys, uint32_t *out_counts,
                                           uint64_t *bucket_unique, hipStream_t s, bool ordered) {
    if (!nlist) return hipSuccess;
    if (k > 63 || k <= 32) return hipErrorInvalidValue;
    constexpr uint32_t MC = WAVE128_MID_CAP, MS_ = WAVE128_MID_CAP * 3 / 2;
#define FK_W128M(MS, ORD)                                                                                       \
    k_bucket_count128_wave<1, MS_, MS, MC, ORD><<<(unsigned)nlist, 64, 0, s>>>(src, buckets, nlist, k, out_keys, \
                                                                              out_counts, bucket_unique, list)
    if (src.np > 0 && ordered)
        FK_W128M(true, true);
    else if (src.np > 0)
        FK_W128M(true, false);
    else if (ordered)
        FK_W128M(false, true);
    else
        FK_W128M(false, false);
#undef FK_W128M
    return hipGetLastError();
}

// 3 / 2 * W2CAP slots per table (as the 64-bit tier: at most 2/3 full)
hipError_t launch_bucket_count128_wave(const BucketSrc &src, const Bucket *buckets, uint64_t nbuckets, int k,
                                       uint64_t *out_keys, uint32_t *out_counts, uint64_t *bucket_unique,
                                       hipStream_t s, bool ordered) {
    if (!nbuckets) return hipSuccess;
    if (k > 63 || k <= 32) return hipErrorInvalidValue;
    const unsigned g = (unsigned)((nbuckets + 1) / 2);
#define FK_W128(MS, ORD)                                                                                   \
    k_bucket_count128_wave<2, W2CAP * 3 / 2, MS, W2CAP, ORD, true><<<g, 64, 0, s>>>(                   \
        src, buckets, nbuckets, k, out_keys, out_counts, bucket_unique)
    if (src.np > 0 && ordered)
        FK_W128(true, true);
    else if (src.np > 0)
        FK_W128(true, false);
    else if (ordered)
        FK_W128(false, true);
    else
        FK_W128(false, false);
#undef FK_W128
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// 5a''''. heavy buckets of 128-bit keys (33 <= k <= 63) split into wave-sized sub-buckets, as
//      k_bucket_split64 / k_sub_count64_seq above: a k = 55 bin's minimizer-prefix clusters fill
//      buckets above the mid wave tier's 512 keys too, which round 4's LDS radix sort and streaming
//      path counted.  Sampled splitters (16 samples per ~SPL_TGT-key sub-bucket, bitonic-sorted in
//      LDS as 128-bit values) cut each bucket into ascending key ranges; the keys are copied in
//      sub-bucket order ((hi, lo) word pairs), then one wave per bucket counts its sub-buckets in
//      order with the mid wave tier's 512-key table (768 slots), each sub-bucket's distinct keys
//      straight after the previous ones'.  A sub-bucket above 512 keys (a k-mer repeated that often)
//      leaves its bucket to the LDS sort (<= block_cap keys) or the streaming path.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_bucket_split128(BucketSrc src, const Bucket *__restrict__ buckets,
                                                        const uint32_t *__restrict__ list, const uint64_t *__restrict__ sbase,
                                                        uint64_t *__restrict__ skeys, SubBucket128 *__restrict__ subs,
                                                        SplitParent *__restrict__ parents, unsigned int *counts,
                                                        uint32_t *__restrict__ fb0, uint32_t *__restrict__ fb1,
                                                        uint32_t block_cap, int sh, int retry) {
    __shared__ u128 s_smp[WSPL_SMAX];  // the sample, sorted; then the splitters (16 KB)
    __shared__ uint32_t s_cnt[WSPL_MAXS];
    const uint32_t lane = threadIdx.x;
    const uint32_t i = blockIdx.x;
    const uint32_t q = list[i];
    const Bucket b = buckets[q];
    const BucketView v =
        (src.np > 0 && src.starts) ? bucket_view_starts<2>(src, src.starts[q]) : bucket_view<2>(src, b);
    auto key_at = [&](uint32_t j) {
        const uint64_t *p = bucket_key_ptr<2>(v, j);
        return ((u128)p[0] << 64) | p[1];
    };
    uint32_t ns0 = (b.n + SPL_TGT - 1) / SPL_TGT;
    ns0 = ns0 < WSPL_MAXS ? ns0 : WSPL_MAXS;
    // an oversized sub-bucket: cut again from another sample into twice as many (as k_bucket_split64)
    uint32_t ns = ns0, nsp = 0, S = 64;
    const uint32_t c0 = lane * WSPL_PER;
    uint32_t cv[WSPL_PER], sum = 0, ne = 0, big = 0, isum = 0, ine = 0, netot = 0, bigmax = 0;
    auto sub_of = [&](u128 x) {  // the splitters below x
        uint32_t lo = 0, len = nsp;
        while (len > 0) {
            const uint32_t half = len >> 1;
            if (s_smp[lo + half] < x) lo += half + 1, len -= half + 1;
            else len = half;
        }
        return lo;
    };
    for (int att = 0; att < 2; ++att) {
        if (att) {  // uniform: the retry
            ns = 2 * ns0 < WSPL_MAXS ? 2 * ns0 : WSPL_MAXS;
            wave_lds_sync();
        }
        S = 64;
        while (S < ns * SPL_OVER && S < WSPL_SMAX) S <<= 1;
        // 1. the sample, spread over the bucket's copy order (the retry's half a stride later),
        //    bitonic-sorted in LDS by the wave
        const uint64_t soff = att ? (uint64_t)b.n / (2 * S) : 0;
        for (uint32_t j = lane; j < S; j += 64) s_smp[j] = key_at((uint32_t)(((uint64_t)j * b.n) / S + soff));
        for (uint32_t t = lane; t < WSPL_MAXS; t += 64) s_cnt[t] = 0;
        wave_lds_sync();
        for (uint32_t kk = 2; kk <= S; kk <<= 1) {
            for (uint32_t j = kk >> 1; j > 0; j >>= 1) {
                for (uint32_t t = lane; t < S / 2; t += 64) {
                    const uint32_t a = ((t & ~(j - 1)) << 1) | (t & (j - 1)), c = a + j;
                    const u128 x = s_smp[a], y = s_smp[c];
                    if ((x > y) == ((a & kk) == 0)) s_smp[a] = y, s_smp[c] = x;
                }
                wave_lds_sync();
            }
        }
        // 2. splitters: sample (t + 1) * S / ns - 1 for t < ns - 1, to the front
        nsp = ns - 1;
        u128 spv[WSPL_PER];
#pragma unroll
        for (int r = 0; r < WSPL_PER; ++r) {
            const uint32_t t = r * 64 + lane;
            if (t < nsp) spv[r] = s_smp[((uint64_t)(t + 1) * S) / ns - 1];
        }
        wave_lds_sync();
#pragma unroll
        for (int r = 0; r < WSPL_PER; ++r) {
            const uint32_t t = r * 64 + lane;
            if (t < nsp) s_smp[t] = spv[r];
        }
        wave_lds_sync();
        // 3. keys per sub-bucket
        for (uint32_t j0 = 0; j0 < b.n; j0 += 64 * WSPL_KB) {
            u128 x[WSPL_KB];
#pragma unroll
            for (int r = 0; r < WSPL_KB; ++r) {
                const uint32_t j = j0 + r * 64 + lane;
                x[r] = j < b.n ? key_at(j) : (u128)0;
            }
#pragma unroll
            for (int r = 0; r < WSPL_KB; ++r)
                if (j0 + r * 64 + lane < b.n) atomicAdd(&s_cnt[sub_of(x[r])], 1u);
        }
        wave_lds_sync();
        // 4. offsets, non-empty sub-buckets, the largest
        sum = 0, ne = 0, big = 0;
#pragma unroll
        for (int t = 0; t < WSPL_PER; ++t) {
            cv[t] = s_cnt[c0 + t];
            sum += cv[t];
            ne += cv[t] ? 1u : 0u;
            big = cv[t] > big ? cv[t] : big;
        }
        isum = wave_incl_sum<uint32_t>(sum), ine = wave_incl_sum<uint32_t>(ne);
        netot = (uint32_t)__shfl((int)ine, 63, 64);
        bigmax = (uint32_t)__shfl((int)wave_incl_max<uint32_t>(big), 63, 64);
        if ((bigmax <= WAVE128_MID_CAP && !(retry && att == 0)) || ns0 >= WSPL_MAXS) break;  // uniform
    }
    if (bigmax > WAVE128_MID_CAP) {  // uniform: a sub-bucket too large for the wave table
        if (lane == 0) {
            parents[i] = SplitParent{0u, 0u};
            if (b.n <= block_cap)
                fb0[atomicAdd(&counts[1], 1u)] = q;
            else
                fb1[atomicAdd(&counts[2], 1u)] = q;
        }
        return;
    }
    uint32_t first = 0;
    if (lane == 0) first = atomicAdd(&counts[0], netot);
    first = (uint32_t)__shfl((int)first, 0, 64);
    if (lane == 0) parents[i] = SplitParent{first, netot};
    const uint64_t sb = sbase[i];
    const u128 klo = (u128)b.c0 << sh, khi = ((u128)b.c1 << sh) - 1;  // 2k <= 126 bits: no wrap
    uint32_t off = isum - sum, nei = ine - ne;
#pragma unroll
    for (int t = 0; t < WSPL_PER; ++t) {
        const uint32_t sidx = c0 + t, c = cv[t];
        if (c) {
            const u128 lo = sidx == 0 ? klo : s_smp[sidx - 1] + 1;
            const u128 hi = sidx == nsp ? khi : s_smp[sidx];
            const u128 d = hi - lo;
            SubBucket128 e;
            e.src = sb + off;
            e.lo_hi = (uint64_t)(lo >> 64);
            e.lo_lo = (uint64_t)lo;
            e.n = c;
            e.span = hi <= lo ? 0u
                              : ((uint64_t)(d >> 64) ? 128u - (uint32_t)__builtin_clzll((uint64_t)(d >> 64))
                                                     : 64u - (uint32_t)__builtin_clzll((uint64_t)d));
            subs[first + nei] = e;
            ++nei;
        }
        s_cnt[sidx] = off;
        off += c;
    }
    wave_lds_sync();
    // 5. the keys in sub-bucket order, (hi, lo) pairs
    for (uint32_t j0 = 0; j0 < b.n; j0 += 64 * WSPL_KB) {
        u128 x[WSPL_KB];
#pragma unroll
        for (int r = 0; r < WSPL_KB; ++r) {
            const uint32_t j = j0 + r * 64 + lane;
            x[r] = j < b.n ? key_at(j) : (u128)0;
        }
#pragma unroll
        for (int r = 0; r < WSPL_KB; ++r)
            if (j0 + r * 64 + lane < b.n) {
                const uint64_t at = sb + atomicAdd(&s_cnt[sub_of(x[r])], 1u);
                skeys[2 * at] = (uint64_t)(x[r] >> 64);
                skeys[2 * at + 1] = (uint64_t)x[r];
            }
    }
}

hipError_t launch_bucket_split128(const BucketSrc &src, const Bucket *buckets, const uint32_t *list, uint32_t nl,
                                  const uint64_t *sbase, uint64_t *skeys, SubBucket128 *subs, SplitParent *parents,
                                  unsigned int *counts, uint32_t *fb0, uint32_t *fb1, uint32_t block_cap, int k, int F,
                                  hipStream_t s, bool retry) {
    if (!nl) return hipSuccess;
    k_bucket_split128<<<nl, 64, 0, s>>>(src, buckets, list, sbase, skeys, subs, parents, counts, fb0, fb1, block_cap,
                                        2 * k - F, retry ? 1 : 0);
    return hipGetLastError();
}

// One wave per split bucket of 128-bit keys, its sub-buckets counted in order (the next one's keys
// loaded while the current one is counted), the distinct keys of sub-bucket j straight after those
// of sub-buckets 0 .. j - 1.  list[i] = the bucket of parents[i].
template <bool ORD>
__global__ __launch_bounds__(64) void k_sub_count128_seq(const Bucket *__restrict__ buckets,
                                                         const uint32_t *__restrict__ list,
                                                         const SplitParent *__restrict__ parents,
                                                         const SubBucket128 *__restrict__ subs,
                                                         const uint64_t *__restrict__ skeys,
                                                         uint64_t *__restrict__ out_keys,
                                                         uint32_t *__restrict__ out_counts,
                                                         uint64_t *__restrict__ bucket_unique) {
    constexpr uint32_t CAP = WAVE128_MID_CAP, SL = WAVE128_MID_CAP * 3 / 2;
    constexpr int W2KPT = CAP / 64;
    typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));
    __shared__ __attribute__((aligned(16))) WaveLds128<CAP, SL> w;
    const SplitParent P = parents[blockIdx.x];
    if (P.nsub == 0) return;  // left to the LDS sort / streaming path
    const uint32_t q = list[blockIdx.x];
    const uint64_t begin = buckets[q].begin;
    const int lane = threadIdx.x & 63;
    const u64x2 *sk2 = reinterpret_cast<const u64x2 *>(skeys);
    SubBucket128 d0 = subs[P.first], d1;
    uint64_t ah[W2KPT], al[W2KPT], bh[W2KPT], bl[W2KPT];
#pragma unroll
    for (int jj = 0; jj < W2KPT; ++jj) {
        const uint32_t i = jj * 64 + lane;
        const u64x2 x = i < d0.n ? __builtin_nontemporal_load(sk2 + d0.src + i) : u64x2{EMPTY_KEY, EMPTY_KEY};
        ah[jj] = x.x;
        al[jj] = x.y;
    }
    uint64_t pre = 0;
    for (uint32_t j = 0;; ++j) {
        const bool more = j + 1 < P.nsub;
        if (more) {
            d1 = subs[P.first + j + 1];
#pragma unroll
            for (int jj = 0; jj < W2KPT; ++jj) {
                const uint32_t i = jj * 64 + lane;
                const u64x2 x = i < d1.n ? __builtin_nontemporal_load(sk2 + d1.src + i) : u64x2{EMPTY_KEY, EMPTY_KEY};
                bh[jj] = x.x;
                bl[jj] = x.y;
            }
        }
        pre += wave_count_keys128<CAP, SL, ORD>(w, begin + pre, d0.n, ((u128)d0.lo_hi << 64) | d0.lo_lo,
                                                (int)d0.span, 0, ah, al, out_keys, out_counts, nullptr);
        if (!more) break;
        d0 = d1;
#pragma unroll
        for (int jj = 0; jj < W2KPT; ++jj) ah[jj] = bh[jj], al[jj] = bl[jj];
    }
    if (lane == 0) bucket_unique[q] = pre;
}

hipError_t launch_sub_count128_seq(const Bucket *buckets, const uint32_t *list, uint32_t nl, const SplitParent *parents,
                                   const SubBucket128 *subs, const uint64_t *skeys, uint64_t *out_keys,
                                   uint32_t *out_counts, uint64_t *bucket_unique, hipStream_t s, bool ordered) {
    if (!nl) return hipSuccess;
    if (ordered)
        k_sub_count128_seq<true><<<nl, 64, 0, s>>>(buckets, list, parents, subs, skeys, out_keys, out_counts,
                                                   bucket_unique);
    else
        k_sub_count128_seq<false><<<nl, 64, 0, s>>>(buckets, list, parents, subs, skeys, out_keys, out_counts,
                                                    bucket_unique);
    return hipGetLastError();
}
