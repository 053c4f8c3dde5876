// fk_query.inc: k-mer count lookups in the sorted count's result -- included by fk_kernels.hip
// inside namespace fk.
// ---------------------------------------------------------------------------
// 7. lookups (fk_query*, no reference counterpart; their host side is fk_views.cpp).  The result
//    stays bucket-major (the count's sorted_result, fk_api.cpp): bucket q holds the cells [c0, c1) of
//    one local bin, its distinct keys lie ascending at res_keys + KW * begin with their counts at
//    out_counts + begin, dense_off[q + 1] - dense_off[q] of them (a heavy bucket's sub-buckets are
//    written in splitter order one after the other, k_sub_count64_seq / k_sub_count128_seq, so the
//    whole bucket ascends).  One lane per query:
//      key -> reverse complement -> canonical key, signature (kmer_signature) -> bin -> owner and
//      local bin -> cell = top F bits -> g = (lbin << F) + cell -> bucket -> binary search.
//    The bucket of cell g: flag_scan is the exclusive scan of the bucket-start flags with the
//    total behind it, so flag_scan[g + 1] counts the buckets that start at or before g, and every
//    bin's cell 0 starts one: q = flag_scan[g + 1] - 1.  The Bucket's own lbin / c0 / c1 then
//    decide whether the cell is its (the lookup trusts them, not the arithmetic).
//    Per query: 8 * KW bytes of key in, 4 (+ 4) bytes out, and a chain of dependent loads --
//    [owner table] -> flag_scan -> (Bucket | dense_off pair) -> ~log2(distinct keys of the bucket)
//    keys -> one count.  Nothing is staged in LDS and the kernel keeps few registers: it hides the
//    chain's latency by occupancy alone.
// ---------------------------------------------------------------------------

template <int KW>
__device__ __forceinline__ KmerKey query_load_key(const uint64_t *__restrict__ p, uint64_t i) {
    if constexpr (KW == 2)
        return KmerKey{p[2 * i], p[2 * i + 1]};
    else
        return KmerKey{0, p[i]};
}

// the count of canonical key c of bin `bin` (0: absent, or the bin is another rank's)
template <int KW>
__device__ __forceinline__ uint32_t query_count(const QueryTables &t, const KmerKey &c, uint32_t bin) {
    uint32_t lbin;
    if (t.owner) {
        if (t.owner[bin] != t.rank) return 0;
        lbin = t.local[bin];
    } else {
        const uint32_t d = bin / t.G;
        if (bin - d * t.G != t.rank) return 0;
        lbin = d;
    }
    if (lbin >= t.nlb) return 0;
    const uint32_t cell = key_cell(c, t.k, t.F);
    const uint64_t g = ((uint64_t)lbin << t.F) + cell;
    uint64_t q = t.flag_scan[g + 1];
    if (q == 0 || q > t.nbuckets) return 0;
    --q;
    const Bucket b = t.buckets[q];
    const uint64_t d0 = t.dense_off[q], d1 = t.dense_off[q + 1];
    if (b.lbin != lbin || cell < b.c0 || cell >= b.c1) return 0;
    const uint64_t *__restrict__ kp = t.keys + KW * b.begin;
    uint32_t lo = 0, hi = (uint32_t)(d1 - d0);
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        const KmerKey x = query_load_key<KW>(kp, mid);
        if (x.lo == c.lo && x.hi == c.hi) return t.counts[b.begin + mid];
        if (key_less(x, c))
            lo = mid + 1;
        else
            hi = mid;
    }
    return 0;
}

// a key on either strand -> (count, bin); (0, -1) for a key with a bit above 2k - 1
template <int KW>
__device__ __forceinline__ void query_one(const QueryTables &t, const KmerKey &f, uint32_t &count, int32_t &bin) {
    count = 0;
    bin = -1;
    if (!key_is_kmer(f, t.k)) return;
    const KmerKey r = revcomp_key<KW == 2>(f, t.k);
    const uint32_t b = bin_of_signature(kmer_signature<KW == 2>(f, r, t.k, t.m), t.fm);
    bin = (int32_t)b;
    count = query_count<KW>(t, key_less(r, f) ? r : f, b);
}

template <int KW>
__global__ __launch_bounds__(NT) void k_query(QueryTables t, const uint64_t *__restrict__ keys, uint64_t n,
                                              uint32_t *__restrict__ counts, int32_t *__restrict__ bins) {
    const uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    uint32_t cnt;
    int32_t bin;
    query_one<KW>(t, query_load_key<KW>(keys, i), cnt, bin);
    counts[i] = cnt;
    if (bins) bins[i] = bin;
}

// window i of a base sequence = seq[i, i + k): packed here (2 bits per base, first base highest),
// then the same lookup; a window holding a byte that is no A/C/G/T counts 0
template <int KW>
__global__ __launch_bounds__(NT) void k_query_seq(QueryTables t, const uint8_t *__restrict__ seq, uint64_t nwin,
                                                  uint32_t *__restrict__ counts) {
    const uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= nwin) return;
    KmerKey f{0, 0};
    uint32_t bad = 0;
    for (int j = 0; j < t.k; ++j) {
        const uint32_t code = base_code(seq[i + j]);
        bad |= code >> 2;
        if constexpr (KW == 2) f.hi = (f.hi << 2) | (f.lo >> 62);
        f.lo = (f.lo << 2) | (code & 3u);
    }
    uint32_t cnt = 0;
    int32_t bin = -1;
    if (!bad) query_one<KW>(t, f, cnt, bin);
    counts[i] = cnt;
}

hipError_t launch_query(int KW, const QueryTables &t, const uint64_t *keys, uint64_t n, uint32_t *counts,
                        int32_t *bins, hipStream_t s) {
    if (!n) return hipSuccess;
    if ((n + NT - 1) / NT > 0x7fffffffull) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)((n + NT - 1) / NT);
    if (KW == 1)
        k_query<1><<<grid, NT, 0, s>>>(t, keys, n, counts, bins);
    else
        k_query<2><<<grid, NT, 0, s>>>(t, keys, n, counts, bins);
    return hipGetLastError();
}

hipError_t launch_query_seq(int KW, const QueryTables &t, const uint8_t *seq, uint64_t nwin, uint32_t *counts,
                            hipStream_t s) {
    if (!nwin) return hipSuccess;
    if ((nwin + NT - 1) / NT > 0x7fffffffull) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)((nwin + NT - 1) / NT);
    if (KW == 1)
        k_query_seq<1><<<grid, NT, 0, s>>>(t, seq, nwin, counts);
    else
        k_query_seq<2><<<grid, NT, 0, s>>>(t, seq, nwin, counts);
    return hipGetLastError();
}
