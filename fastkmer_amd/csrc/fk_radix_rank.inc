// fk_radix_rank.inc -- included by fk_kernels.hip inside namespace fk.
// Stable block-wide ranking of one LSD radix digit (4 bits) for a tile of
// keys in blocked arrangement; shared by the LDS bucket counters and the
// large-bucket path.

template <int KW>
__device__ __forceinline__ uint32_t digit_of(uint64_t key, int sh) { return (uint32_t)(key >> sh) & 15u; }
template <int KW>
__device__ __forceinline__ uint32_t digit_of(u128 key, int sh) { return (uint32_t)(key >> sh) & 15u; }

// the bits a bucket sort orders by: a 64-bit staged key's k-mer (WKeySpec: the weight field above it
// is payload), every bit of a 128-bit key
template <int KW>
__device__ __forceinline__ typename KeyOf<KW>::T sort_kmask(int k) {
    typedef typename KeyOf<KW>::T K;
    if constexpr (KW == 1) return 2 * k <= WKEY_MAX_BITS ? (1ull << (2 * k)) - 1ull : ~0ull;
    else return ~(K)0;
}

// Rank one tile of up to NT*IPT keys (blocked arrangement: thread t owns
// items [t*IPT, t*IPT+IPT), items >= n inactive).  Returns, per item, its
// position in the stable order by digit inside the tile; s_cnt is 16*NT u32.
template <typename K, int IPT>
__device__ __forceinline__ void tile_rank(const K (&key)[IPT], int n_valid_here, int sh, uint32_t *s_cnt,
                                          uint32_t *s_tmp, uint32_t (&pos)[IPT], uint32_t (&dig)[IPT],
                                          uint32_t *digit_total /*[16] or null*/, uint32_t dmask = 15u) {
    // dmask: the digit's bits that count (a weighted key's top digit stops at the k-mer's last bit)
    uint64_t lo = 0, hi = 0;  // 16 counters x 8 bits
#pragma unroll
    for (int it = 0; it < IPT; ++it) {
        const uint32_t d = (uint32_t)(key[it] >> sh) & dmask;
        dig[it] = d;
        if (it < n_valid_here) {
            const int f = 8 * (d & 7);
            const uint64_t word = (d < 8) ? lo : hi;
            pos[it] = (uint32_t)(word >> f) & 0xffu;  // rank among this thread's items with digit d
            if (d < 8)
                lo += 1ull << f;
            else
                hi += 1ull << f;
        }
    }
    // counts to LDS in (digit, thread) order
#pragma unroll
    for (int d = 0; d < 16; ++d) {
        const uint64_t word = d < 8 ? lo : hi;
        s_cnt[d * NT + threadIdx.x] = (uint32_t)(word >> (8 * (d & 7))) & 0xffu;
    }
    __syncthreads();
    // exclusive scan over the 16*NT counters: thread t scans entries [16t, 16t+16)
    uint32_t v[16];
    uint32_t sum = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        v[j] = s_cnt[threadIdx.x * 16 + j];
        sum += v[j];
    }
    uint32_t tot;
    uint32_t run = block_excl_sum<uint32_t>(sum, s_tmp, &tot);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        s_cnt[threadIdx.x * 16 + j] = run;
        run += v[j];
    }
    __syncthreads();
    if (digit_total && threadIdx.x < 16) {
        const uint32_t st = s_cnt[threadIdx.x * NT];
        const uint32_t en = threadIdx.x < 15 ? s_cnt[(threadIdx.x + 1) * NT] : tot;
        digit_total[threadIdx.x] = en - st;
    }
#pragma unroll
    for (int it = 0; it < IPT; ++it)
        if (it < n_valid_here) pos[it] += s_cnt[dig[it] * NT + threadIdx.x];
}

