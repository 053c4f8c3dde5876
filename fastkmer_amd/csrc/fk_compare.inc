// fk_compare.inc: two counted results compared on the device -- included by fk_kernels.hip inside
// namespace fk.
// ---------------------------------------------------------------------------
// 9. two-sample comparison (fk_compare*, fk_*_joined, no reference counterpart).  Result A (`a`,
//    walked) and result B (`b`, looked up in) are two contexts' bucket-major results of the sorted
//    count, as QueryTables: the same k, m, bin count, ranks, rank and bin owners, but each with its
//    own buckets and its own cell bits F.  Every kernel walks A bucket by bucket, one wave per
//    bucket in 64-wide strips (fk_spectrum.inc): lane i of a strip holds A's key src + i and its
//    count ca, and looks the key up in B with query_count (fk_query.inc).
//    What the lookup takes from A: the key is canonical already.  Its bin is the bucket's, and every key
//    of a bucket lies in one bin, so the signature is recomputed as query_one does, but once per bucket,
//    from the bucket's first key (bucket_bin).  That needs no local-bin -> bin table under a size-aware
//    placement, and it keeps the signature's ~700 instructions (k = 28) out of the per-key path: with one
//    signature per key the two walks of profiles/compare_rate.txt took 7.60 ms instead of 6.65 (before the tuning below).
//    Nothing else is taken: B's cell is key_cell(c, k, b.F) with B's F inside query_count, A's cell index
//    means nothing in B.
//
//    Joint matrix M[rows][cols] (row-major, uint64): the A-walk adds every k-mer of A at
//    M[min(ca, rows - 1)][min(cb, cols - 1)], cb = 0 for a k-mer B lacks.  The B-walk is the same
//    kernel with the tables swapped and only_absent set: a k-mer of B found in A was counted by the
//    A-walk and adds nothing, one absent from A adds at M[0][min(cb, cols - 1)].  M[0][0] stays 0.
//    Where the adds go (sequencing data piles onto M[1][0], M[0][1] and the diagonal at the coverage
//    peaks, and one global atomic per lane would serialise there as on the spectrum's hist[1]):
//      - the singletons absent from the other side, (1, 0) / (0, 1), in a per-lane register: a
//        compare and an add, summed over the wave once at the end (SPEC_WAVE's reasoning),
//      - entries below CMP_TILE on both axes in a workgroup-private LDS tile, one LDS atomic per lane;
//        the persistent grid flushes a tile's nonzero entries once per workgroup,
//      - everything else by device-scope global atomics: rare (counts >= CMP_TILE on either side).
//    LT, the tile's entries and the lane counter: 32-bit when the walked result holds fewer than 2^32
//    k-mers (each adds 1 per k-mer), else 64-bit.
//    The kernel is bound by the lookups' chains of dependent loads (flag_scan -> Bucket / dense_off ->
//    ~log2(bucket) keys -> count), which occupancy hides: a 16 KB tile leaves LDS room for 8
//    workgroups per CU, all 32 wave slots.  Neighbouring lanes hold ascending neighbours of one
//    bucket, so their binary searches in B share their upper probes (one cache line per probe level
//    for most of the wave).  A search loop is data dependent, so the strips of a wave cannot overlap
//    their lookups; a wave loads CMP_STRIPS strips of keys and counts before it looks the first up.
// ---------------------------------------------------------------------------

// Tuning constants, measured at the two configs[1]-parameter samples of profiles/compare_rate.txt (82 M
// distinct k-mers each, half of the reads shared; both walks of a 256 x 256 matrix, medians of 20 calls
// by device events, one constant changed at a time).
// The LDS tile holds M[0 .. CMP_TILE)[0 .. CMP_TILE): 16 KB (32 KB for 64-bit entries), eight workgroups
// per CU.  32: 6.70 ms, 64: 6.65, 128 (64 KB, two workgroups per CU): 11.43 -- before the occupancy
// below was forced; the sample's counts stop at 13, so the tile's reach did not matter, its size did.
constexpr uint32_t CMP_TILE = 64;
// Persistent grid: 8 workgroups per CU (SPEC_GRID's), every wave slot once.  1024: 6.83 ms, 2048: 4.09,
// 16384: 4.19.
constexpr unsigned CMP_GRID = 2048;
// 64-key strips a wave loads before it looks them up.  1: 4.29 ms, 2: 4.09, 4: 4.04 (a result against
// itself, one walk: 1.96 / 1.66 / 1.53).
constexpr int CMP_STRIPS = 4;
// Waves per SIMD.  Left to the compiler the kernel held two QueryTables in more scalar registers than
// eight waves per SIMD may have and ran seven: 2048 workgroups then need a second round for their last
// eighth (6.65 ms; larger grids hid it in part: 4096: 5.33, 8192: 5.19, 16384: 5.13).  With eight waves
// forced: 4.11 ms at the same grid.  (The 64-bit tile's 32 KB allow four workgroups per CU: four waves.)
template <typename LT>
constexpr int cmp_waves() { return sizeof(LT) == 4 ? 8 : 4; }

// the bin of a's bucket whose first key is at `src` (it holds one at least): query_one's signature of
// that key and its reverse complement, the same in every lane
template <int KW>
__device__ __forceinline__ uint32_t bucket_bin(const QueryTables &a, uint64_t src) {
    const KmerKey c = query_load_key<KW>(a.keys, src);
    const KmerKey r = revcomp_key<KW == 2>(c, a.k);
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)bin_of_signature(kmer_signature<KW == 2>(c, r, a.k, a.m), a.fm));
}

// M zeroed by the launcher (the A-walk's).  a: the walked result, b: the looked-up one.  only_absent =
// false: M[min(ca, rows - 1)][min(cb, cols - 1)] += 1 per k-mer of a; true (a and b swapped by the
// caller, M's axes are not): M[0][min(ca, cols - 1)] += 1 per k-mer of a that b lacks.
template <int KW, typename LT>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(cmp_waves<LT>(), 8)))
void k_compare(QueryTables a, QueryTables b, unsigned long long *__restrict__ M, uint32_t rows, uint32_t cols,
               bool only_absent) {
    __shared__ LT s_tile[CMP_TILE * CMP_TILE];
    __shared__ unsigned long long s_single;  // the waves' register counters summed
    for (uint32_t i = threadIdx.x; i < CMP_TILE * CMP_TILE; i += NT) s_tile[i] = 0;
    if (threadIdx.x == 0) s_single = 0ull;
    __syncthreads();
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const uint64_t stride = (uint64_t)gridDim.x * (NT / 64);
    const uint32_t rmax = rows - 1, cmax = cols - 1;
    LT single = 0;  // per lane: k-mers of count 1 the other result lacks
    for (uint64_t q = (uint64_t)blockIdx.x * (NT / 64) + wid; q < a.nbuckets; q += stride) {
        const uint64_t src = a.buckets[q].begin;
        const uint64_t nu = a.dense_off[q + 1] - a.dense_off[q];
        if (nu == 0) continue;
        const uint32_t bin = bucket_bin<KW>(a, src);
        for (uint64_t i = 0; i < nu; i += 64 * CMP_STRIPS) {
            KmerKey key[CMP_STRIPS];
            uint32_t cs[CMP_STRIPS];
#pragma unroll
            for (int j = 0; j < CMP_STRIPS; ++j) {
                const uint64_t p = i + 64u * j + lane;
                const bool valid = p < nu;
                key[j] = query_load_key<KW>(a.keys, valid ? src + p : src);  // nu >= 1: the bucket's first key exists
                cs[j] = valid ? a.counts[src + p] : 0u;                      // no k-mer of a result has count 0
            }
#pragma unroll
            for (int j = 0; j < CMP_STRIPS; ++j) {
                if (!cs[j]) continue;
                const uint32_t co = query_count<KW>(b, key[j], bin);
                if (only_absent && co) continue;
                if (co == 0 && cs[j] == 1) {
                    single += 1;
                    continue;
                }
                const uint32_t r = only_absent ? 0u : (cs[j] < rmax ? cs[j] : rmax);
                const uint32_t cv = only_absent ? cs[j] : co;
                const uint32_t c = cv < cmax ? cv : cmax;
                if (r < CMP_TILE && c < CMP_TILE)
                    atomicAdd(&s_tile[r * CMP_TILE + c], (LT)1);
                else
                    atomicAdd(&M[(uint64_t)r * cols + c], 1ull);
            }
        }
    }
    const uint64_t sw = wave_sum_u64((uint64_t)single);
    if (lane == 0 && sw) atomicAdd(&s_single, (unsigned long long)sw);
    __syncthreads();
    // an entry was added to only with r <= rows - 1 and c <= cols - 1: a nonzero one lies inside M
    for (uint32_t i = threadIdx.x; i < CMP_TILE * CMP_TILE; i += NT) {
        const unsigned long long v = (unsigned long long)s_tile[i];
        if (v) atomicAdd(&M[(uint64_t)(i / CMP_TILE) * cols + i % CMP_TILE], v);
    }
    // rows, cols >= 2: (1, 0) and (0, 1) are never clamped
    if (threadIdx.x == 0 && s_single) atomicAdd(&M[only_absent ? 1ull : (uint64_t)cols], s_single);
}

static unsigned compare_grid(uint64_t nbuckets) {
    return (unsigned)std::min<uint64_t>((nbuckets + NT / 64 - 1) / (NT / 64), CMP_GRID);
}

hipError_t launch_compare(int KW, const QueryTables &a, const QueryTables &b, uint64_t distinct, uint64_t *M,
                          uint32_t rows, uint32_t cols, bool only_absent, hipStream_t s) {
    if (rows < 2 || cols < 2) return hipErrorInvalidValue;
    if (!only_absent) {
        const hipError_t e = hipMemsetAsync(M, 0, (uint64_t)rows * cols * 8, s);
        if (e != hipSuccess) return e;
    }
    if (!a.nbuckets) return hipSuccess;
    const unsigned grid = compare_grid(a.nbuckets);
    unsigned long long *m = reinterpret_cast<unsigned long long *>(M);
    const bool wide = (distinct >> 32) != 0;
    if (KW == 1) {
        if (wide)
            k_compare<1, unsigned long long><<<grid, NT, 0, s>>>(a, b, m, rows, cols, only_absent);
        else
            k_compare<1, uint32_t><<<grid, NT, 0, s>>>(a, b, m, rows, cols, only_absent);
    } else {
        if (wide)
            k_compare<2, unsigned long long><<<grid, NT, 0, s>>>(a, b, m, rows, cols, only_absent);
        else
            k_compare<2, uint32_t><<<grid, NT, 0, s>>>(a, b, m, rows, cols, only_absent);
    }
    return hipGetLastError();
}

// ---- joined views: a k-mer of a is kept when lo <= ca <= hi and olo <= cb <= ohi (cb = 0: b lacks it)

struct JoinRange {
    uint32_t lo, hi, olo, ohi;
};

// the one predicate of the count pass and the compact pass: cb is looked up only for a k-mer whose own
// count passes, and is valid only when the k-mer is kept
template <int KW>
__device__ __forceinline__ bool join_keep(const QueryTables &a, const QueryTables &b, const JoinRange &rg, uint32_t bin,
                                          uint64_t at, bool valid, uint32_t &ca, uint32_t &cb) {
    ca = valid ? a.counts[at] : 0u;
    cb = 0;
    if (!valid || ca < rg.lo || ca > rg.hi) return false;
    const KmerKey key = query_load_key<KW>(a.keys, at);
    cb = query_count<KW>(b, key, bin);
    return cb >= rg.olo && cb <= rg.ohi;
}

// kept[q] = kept k-mers of bucket q of a, one wave per bucket
template <int KW>
__global__ __launch_bounds__(NT) void k_join_count(QueryTables a, QueryTables b, JoinRange rg,
                                                   uint64_t *__restrict__ kept) {
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const uint64_t stride = (uint64_t)gridDim.x * (NT / 64);
    for (uint64_t q = (uint64_t)blockIdx.x * (NT / 64) + wid; q < a.nbuckets; q += stride) {
        const uint64_t src = a.buckets[q].begin;
        const uint64_t nu = a.dense_off[q + 1] - a.dense_off[q];
        uint64_t cnt = 0;  // wave-uniform
        const uint32_t bin = nu ? bucket_bin<KW>(a, src) : 0u;
        for (uint64_t i = 0; i < nu; i += 64) {
            uint32_t ca, cb;
            const bool keep = join_keep<KW>(a, b, rg, bin, src + i + lane, i + lane < nu, ca, cb);
            cnt += (uint64_t)__popcll(__ballot(keep));
        }
        if (lane == 0) kept[q] = cnt;
    }
}

// bucket q's kept k-mers in the bucket's order at keep_off[q] of the dense filtered arrays (any of
// which may be null), as k_range_compact places them
template <int KW>
__global__ __launch_bounds__(NT) void k_join_compact(QueryTables a, QueryTables b, JoinRange rg,
                                                     const uint64_t *__restrict__ keep_off,
                                                     uint64_t *__restrict__ fkeys, uint32_t *__restrict__ fcounts,
                                                     uint32_t *__restrict__ fother) {
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const uint64_t stride = (uint64_t)gridDim.x * (NT / 64);
    const uint64_t below = (1ull << lane) - 1ull;
    for (uint64_t q = (uint64_t)blockIdx.x * (NT / 64) + wid; q < a.nbuckets; q += stride) {
        uint64_t base = keep_off[q];
        if (keep_off[q + 1] == base) continue;  // nothing kept
        const uint64_t src = a.buckets[q].begin;
        const uint64_t nu = a.dense_off[q + 1] - a.dense_off[q];
        const uint32_t bin = bucket_bin<KW>(a, src);  // something is kept: the bucket holds a key
        for (uint64_t i = 0; i < nu; i += 64) {
            uint32_t ca, cb;
            const bool keep = join_keep<KW>(a, b, rg, bin, src + i + lane, i + lane < nu, ca, cb);
            const uint64_t mask = __ballot(keep);
            if (keep) {
                const uint64_t d = base + (uint64_t)__popcll(mask & below);
                if (fkeys) {
                    if constexpr (KW == 1) {
                        fkeys[d] = a.keys[src + i + lane];
                    } else {
                        fkeys[2 * d] = a.keys[2 * (src + i + lane)];
                        fkeys[2 * d + 1] = a.keys[2 * (src + i + lane) + 1];
                    }
                }
                if (fcounts) fcounts[d] = ca;
                if (fother) fother[d] = cb;
            }
            base += (uint64_t)__popcll(mask);
        }
    }
}

hipError_t launch_join_count(int KW, const QueryTables &a, const QueryTables &b, uint32_t lo, uint32_t hi,
                             uint32_t olo, uint32_t ohi, uint64_t *kept, hipStream_t s) {
    if (!a.nbuckets) return hipSuccess;
    const JoinRange rg{lo, hi, olo, ohi};
    if (KW == 1)
        k_join_count<1><<<range_grid(a.nbuckets), NT, 0, s>>>(a, b, rg, kept);
    else
        k_join_count<2><<<range_grid(a.nbuckets), NT, 0, s>>>(a, b, rg, kept);
    return hipGetLastError();
}

hipError_t launch_join_compact(int KW, const QueryTables &a, const QueryTables &b, uint32_t lo, uint32_t hi,
                               uint32_t olo, uint32_t ohi, const uint64_t *keep_off, uint64_t *fkeys,
                               uint32_t *fcounts, uint32_t *fother, hipStream_t s) {
    if (!a.nbuckets) return hipSuccess;
    const JoinRange rg{lo, hi, olo, ohi};
    if (KW == 1)
        k_join_compact<1><<<range_grid(a.nbuckets), NT, 0, s>>>(a, b, rg, keep_off, fkeys, fcounts, fother);
    else
        k_join_compact<2><<<range_grid(a.nbuckets), NT, 0, s>>>(a, b, rg, keep_off, fkeys, fcounts, fother);
    return hipGetLastError();
}
