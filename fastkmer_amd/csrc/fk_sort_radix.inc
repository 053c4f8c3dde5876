// fk_sort_radix.inc: stable LDS radix ranking, 128-bit bucket sort and the large-bucket path -- included by fk_kernels.hip inside namespace fk.
// ---------------------------------------------------------------------------
// 5a. bucket sort + run-length count in LDS (quickSort + heap merge of
//     extractKXmers, SBKC:540-597).  LSD radix sort, 4-bit digits, blocked
//     arrangement (thread t owns IPT consecutive keys); per-thread digit
//     counters live in two 64-bit registers (8-bit fields), the block-wide
//     (digit, thread) scan runs over 16 x 256 counters in LDS, so ranks are
//     stable and no LDS atomics are needed.  Only digits whose bits differ
//     inside the bucket are sorted.
// ---------------------------------------------------------------------------

template <int KW>
__global__ __launch_bounds__(NT) void k_bucket_sort(BucketSrc src, const Bucket *__restrict__ buckets, int k,
                                                    uint64_t *__restrict__ out_keys,
                                                    uint32_t *__restrict__ out_counts, uint64_t *bucket_unique,
                                                    unsigned long long *oversize, uint32_t small_limit,
                                                    const uint32_t *__restrict__ list, uint32_t skip_le) {
    typedef typename KeyOf<KW>::T K;
    constexpr int CAP = SORT_CAP / KW;
    constexpr int IPT = CAP / NT;
    __shared__ K s_keys[CAP];
    __shared__ uint32_t s_cnt[16 * NT + 1];
    __shared__ uint32_t s_tmp[NT / 64];
    __shared__ K s_red[2][NT / 64];

    const uint32_t qi = list ? list[blockIdx.x] : blockIdx.x;  // bucket (list: the block tier only)
    const Bucket b = buckets[qi];
    const int n = (int)b.n;
    if (skip_le && b.n <= skip_le) return;  // counted by a wave tier (listed with the block tier)
    if (b.n > (uint32_t)CAP || b.n > small_limit) {
        if (threadIdx.x == 0) {
            bucket_unique[qi] = REDO;
            atomicAdd(oversize, 1ull);
        }
        return;
    }
    if (n == 0) {
        if (threadIdx.x == 0) bucket_unique[qi] = 0;
        return;
    }
    // gather the bucket's runs into LDS, then a blocked load + OR/AND reduction
    {  // one array, or the staged pieces (BucketView)
        const BucketView bv = bucket_view<KW>(src, b);
        for (uint32_t li = threadIdx.x; li < (uint32_t)n; li += NT) {
            K x;
            load_key(bucket_key_ptr<KW>(bv, li), 0, x);
            s_keys[li] = x;
        }
    }
    __syncthreads();
    K key[IPT];
    K kor = 0, kand = ~(K)0;
    const int my0 = threadIdx.x * IPT;
    const int nv = max(0, min(IPT, n - my0));
#pragma unroll
    for (int it = 0; it < IPT; ++it) {
        if (it < nv) {
            key[it] = s_keys[my0 + it];
            kor |= key[it];
            kand &= key[it];
        } else {
            key[it] = ~(K)0;
        }
    }
    {
        const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            if constexpr (KW == 1) {
                kor |= __shfl_xor(kor, d, 64);
                kand &= __shfl_xor(kand, d, 64);
            } else {
                const uint64_t a = (uint64_t)kor, bb = (uint64_t)(kor >> 64);
                const uint64_t c = (uint64_t)kand, e = (uint64_t)(kand >> 64);
                kor |= ((u128)__shfl_xor(bb, d, 64) << 64) | __shfl_xor(a, d, 64);
                kand &= ((u128)__shfl_xor(e, d, 64) << 64) | __shfl_xor(c, d, 64);
            }
        }
        if (lane == 0) {
            s_red[0][wid] = kor;
            s_red[1][wid] = kand;
        }
        __syncthreads();
        kor = s_red[0][0] | s_red[0][1] | s_red[0][2] | s_red[0][3];
        kand = s_red[1][0] & s_red[1][1] & s_red[1][2] & s_red[1][3];
        __syncthreads();
    }
    // 64-bit keys may be weighted (WKeySpec): the digits stop at the k-mer's bits (the sort is stable,
    // so a k-mer's entries end up adjacent whatever their weights), a run's head is a change of k-mer
    // and its count the sum of its entries' weights
    const K kmask = sort_kmask<KW>(k);
    const K diff = (kor ^ kand) & kmask;
    const bool weighted = ((kor & ~kmask) != 0);  // uniform
    int lo_bit = 0, hi_bit = -1;
    if (diff != 0) {
        if constexpr (KW == 1) {
            lo_bit = __builtin_ctzll(diff);
            hi_bit = 63 - __builtin_clzll(diff);
        } else {
            const uint64_t dl = (uint64_t)diff, dh = (uint64_t)(diff >> 64);
            lo_bit = dl ? __builtin_ctzll(dl) : 64 + __builtin_ctzll(dh);
            hi_bit = dh ? 127 - __builtin_clzll(dh) : 63 - __builtin_clzll(dl);
        }
    }
    for (int sh = lo_bit & ~3; sh <= hi_bit; sh += 4) {
        uint32_t pos[IPT], dig[IPT];
        tile_rank<K, IPT>(key, nv, sh, s_cnt, s_tmp, pos, dig, nullptr, (uint32_t)(kmask >> sh) & 15u);
#pragma unroll
        for (int it = 0; it < IPT; ++it)
            if (it < nv) s_keys[pos[it]] = key[it];
        __syncthreads();
#pragma unroll
        for (int it = 0; it < IPT; ++it) key[it] = (it < nv) ? s_keys[my0 + it] : ~(K)0;
        __syncthreads();
    }
    if (hi_bit < 0 && !weighted) {
        // all keys equal
        if (threadIdx.x == 0) {
            store_key(out_keys, b.begin, key[0]);
            out_counts[b.begin] = (uint32_t)n;
            bucket_unique[qi] = 1;
        }
        return;
    }
    // run-length encode: heads -> unique index; head positions in s_cnt
#pragma unroll
    for (int it = 0; it < IPT; ++it) s_keys[my0 + it] = key[it];
    __syncthreads();
    uint32_t heads = 0;
#pragma unroll
    for (int it = 0; it < IPT; ++it) {
        const int i = my0 + it;
        if (i < n && (i == 0 || ((s_keys[i - 1] ^ key[it]) & kmask) != 0)) heads |= 1u << it;
    }
    uint32_t nu;
    uint32_t u = block_excl_sum<uint32_t>((uint32_t)__popc(heads), s_tmp, &nu);
#pragma unroll
    for (int it = 0; it < IPT; ++it)
        if ((heads >> it) & 1u) s_cnt[u++] = (uint32_t)(my0 + it);
    if (threadIdx.x == 0) s_cnt[nu] = (uint32_t)n;
    __syncthreads();
    for (uint32_t q = threadIdx.x; q < nu; q += NT) {
        const uint32_t hp = s_cnt[q];
        store_key(out_keys, b.begin + q, s_keys[hp] & kmask);
        uint32_t cnt = s_cnt[q + 1] - hp;
        if constexpr (KW == 1) {
            if (weighted)  // the run's weights (weight - 1 above the k-mer) on top of its length
                for (uint32_t j = hp, e = hp + cnt; j < e; ++j) cnt += (uint32_t)(s_keys[j] >> (2 * k));
        }
        out_counts[b.begin + q] = cnt;
    }
    if (threadIdx.x == 0) bucket_unique[qi] = nu;
}

hipError_t launch_bucket_sort(int KW, const BucketSrc &src, const Bucket *buckets, uint64_t nbuckets, int k,
                              uint64_t *out_keys, uint32_t *out_counts, uint64_t *bucket_unique,
                              unsigned long long *oversize, uint32_t small_limit, const uint32_t *list, hipStream_t s,
                              uint32_t skip_le) {
    if (!nbuckets) return hipSuccess;
    if (KW == 1)
        k_bucket_sort<1><<<(unsigned)nbuckets, NT, 0, s>>>(src, buckets, k, out_keys, out_counts, bucket_unique,
                                                             oversize, small_limit, list, skip_le);
    else
        k_bucket_sort<2><<<(unsigned)nbuckets, NT, 0, s>>>(src, buckets, k, out_keys, out_counts, bucket_unique,
                                                             oversize, small_limit, list, skip_le);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// 5b. buckets above the LDS capacity: one workgroup streams the bucket in
//     tiles through the same stable ranking (global LSD radix sort with
//     ping-pong between a scratch copy and the bucket's region of out_keys),
//     then run-length encodes.  The scratch copy sits at the bucket's own
//     offset (scratch as large as the keys), or -- with a cursor -- at an offset
//     taken from it (scratch as large as the listed buckets' keys).
// ---------------------------------------------------------------------------

template <int KW>
__global__ __launch_bounds__(NT) void k_bucket_sort_large(BucketSrc src, const Bucket *buckets, int k,
                                                          uint64_t *scratch, uint64_t *out_keys,
                                                          uint32_t *out_counts, uint64_t *bucket_unique,
                                                          const uint32_t *__restrict__ list,
                                                          unsigned long long *scratch_cursor) {
    typedef typename KeyOf<KW>::T K;
    constexpr int IPT = (SORT_CAP / KW) / NT;
    constexpr int TILE = NT * IPT;
    __shared__ uint32_t s_cnt[16 * NT + 1];
    __shared__ uint32_t s_tmp[NT / 64];
    __shared__ uint32_t s_dtot[16];
    __shared__ uint64_t s_dbase[16];
    __shared__ uint64_t s_hist[16];
    __shared__ K s_red[2][NT / 64];
    __shared__ K s_carry;
    __shared__ uint64_t s_state[3];
    __shared__ uint64_t s_soff;

    const uint32_t qi = list ? list[blockIdx.x] : blockIdx.x;
    const Bucket b = buckets[qi];
    if (bucket_unique[qi] != REDO) return;  // counted by the LDS kernels
    const uint64_t n = b.n;
    if (threadIdx.x == 0) s_soff = scratch_cursor ? atomicAdd(scratch_cursor, (unsigned long long)n) : b.begin;
    __syncthreads();
    // gather the bucket's runs into scratch[soff, soff + n)
    const uint64_t soff = s_soff;
    {  // one array, or the staged pieces (BucketView)
        const BucketView bv = bucket_view<KW>(src, b);
        for (uint64_t li = threadIdx.x; li < n; li += NT) {
            K x;
            load_key(bucket_key_ptr<KW>(bv, (uint32_t)li), 0, x);
            store_key(scratch, soff + li, x);
        }
    }
    __syncthreads();
    uint64_t *bufA = scratch, *bufB = out_keys;
    uint64_t offA = soff, offB = b.begin;  // each buffer's first slot of this bucket
    // varying bits
    K kor = 0, kand = ~(K)0;
    for (uint64_t i = threadIdx.x; i < n; i += NT) {
        K x;
        load_key(bufA, offA + i, x);
        kor |= x;
        kand &= x;
    }
    {
        const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
        for (int d = 32; d > 0; d >>= 1) {
            if constexpr (KW == 1) {
                kor |= __shfl_xor(kor, d, 64);
                kand &= __shfl_xor(kand, d, 64);
            } else {
                const uint64_t a = (uint64_t)kor, bb = (uint64_t)(kor >> 64);
                const uint64_t c = (uint64_t)kand, e = (uint64_t)(kand >> 64);
                kor |= ((u128)__shfl_xor(bb, d, 64) << 64) | __shfl_xor(a, d, 64);
                kand &= ((u128)__shfl_xor(e, d, 64) << 64) | __shfl_xor(c, d, 64);
            }
        }
        if (lane == 0) {
            s_red[0][wid] = kor;
            s_red[1][wid] = kand;
        }
        __syncthreads();
        kor = s_red[0][0] | s_red[0][1] | s_red[0][2] | s_red[0][3];
        kand = s_red[1][0] & s_red[1][1] & s_red[1][2] & s_red[1][3];
        __syncthreads();
    }
    // weighted 64-bit keys as in k_bucket_sort: digits up to the k-mer's last bit, heads by k-mer,
    // counts by weight
    const K kmask = sort_kmask<KW>(k);
    const int wsh = KW == 1 && 2 * k <= WKEY_MAX_BITS ? 2 * k : 0;  // 0: no weight field
    const K diff = (kor ^ kand) & kmask;
    int lo_bit = 0, hi_bit = -1;
    if (diff != 0) {
        if constexpr (KW == 1) {
            lo_bit = __builtin_ctzll(diff);
            hi_bit = 63 - __builtin_clzll(diff);
        } else {
            const uint64_t dl = (uint64_t)diff, dh = (uint64_t)(diff >> 64);
            lo_bit = dl ? __builtin_ctzll(dl) : 64 + __builtin_ctzll(dh);
            hi_bit = dh ? 127 - __builtin_clzll(dh) : 63 - __builtin_clzll(dl);
        }
    }
    for (int sh = lo_bit & ~3; sh <= hi_bit; sh += 4) {
        const uint32_t dmask = (uint32_t)(kmask >> sh) & 15u;
        // digit histogram of the whole bucket
        if (threadIdx.x < 16) s_hist[threadIdx.x] = 0;
        __syncthreads();
        for (uint64_t i = threadIdx.x; i < n; i += NT) {
            K x;
            load_key(bufA, offA + i, x);
            atomicAdd((unsigned long long *)&s_hist[(uint32_t)(x >> sh) & dmask], 1ull);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint64_t acc = 0;
            for (int d = 0; d < 16; ++d) {
                s_dbase[d] = acc;  // running base, advanced tile by tile
                acc += s_hist[d];
            }
        }
        __syncthreads();
        for (uint64_t t0 = 0; t0 < n; t0 += TILE) {
            K key[IPT];
            const uint64_t my0 = t0 + (uint64_t)threadIdx.x * IPT;
            const int nv = (int)max((int64_t)0, min((int64_t)IPT, (int64_t)n - (int64_t)my0));
#pragma unroll
            for (int it = 0; it < IPT; ++it) {
                if (it < nv)
                    load_key(bufA, offA + my0 + it, key[it]);
                else
                    key[it] = ~(K)0;
            }
            uint32_t pos[IPT], dig[IPT];
            tile_rank<K, IPT>(key, nv, sh, s_cnt, s_tmp, pos, dig, s_dtot, dmask);
            // pos = position in the tile's digit order; digit d starts at s_cnt[d*NT]
#pragma unroll
            for (int it = 0; it < IPT; ++it) {
                if (it < nv) {
                    const uint32_t d = dig[it];
                    const uint64_t dst = s_dbase[d] + (pos[it] - s_cnt[d * NT]);
                    store_key(bufB, offB + dst, key[it]);
                }
            }
            __syncthreads();
            if (threadIdx.x < 16) s_dbase[threadIdx.x] += s_dtot[threadIdx.x];
            __syncthreads();
        }
        uint64_t *t = bufA;
        bufA = bufB;
        bufB = t;
        const uint64_t to = offA;
        offA = offB;
        offB = to;
        __syncthreads();
    }
    // run-length encode bufA -> out_keys/out_counts.  When bufA == out_keys
    // this compacts in place: a tile is read into registers before any
    // write, and unique index <= position, so later tiles are never clobbered.
    // Counts are differences of the weight before a head (an unweighted key weighs 1: its position)
    if (threadIdx.x == 0) {
        s_state[0] = 0;      // unique keys written so far
        s_state[1] = ~0ull;  // weight before the head whose count is still open
        s_state[2] = 0;      // weight before this tile
    }
    __syncthreads();
    for (uint64_t t0 = 0; t0 < n; t0 += TILE) {
        const uint64_t tlen = min((uint64_t)TILE, n - t0);
        K key[IPT];
        const uint64_t my0 = t0 + (uint64_t)threadIdx.x * IPT;
        const int nv = (int)max((int64_t)0, min((int64_t)IPT, (int64_t)n - (int64_t)my0));
#pragma unroll
        for (int it = 0; it < IPT; ++it) {
            if (it < nv)
                load_key(bufA, offA + my0 + it, key[it]);
            else
                key[it] = ~(K)0;
        }
        K pk;
        if (threadIdx.x == 0)
            pk = s_carry;
        else if (nv > 0)
            load_key(bufA, offA + my0 - 1, pk);
        else
            pk = ~(K)0;
        uint32_t heads = 0, wsum = 0;
        uint32_t wt[IPT];
#pragma unroll
        for (int it = 0; it < IPT; ++it) {
            if (it < nv && ((my0 + it) == 0 || ((key[it] ^ pk) & kmask) != 0)) heads |= 1u << it;
            pk = key[it];
            wt[it] = it < nv ? 1u : 0u;
            if constexpr (KW == 1)
                if (wsh && it < nv) wt[it] += (uint32_t)(key[it] >> wsh);
            wsum += wt[it];
        }
        __syncthreads();  // every read of this tile (and of s_carry) is done
#pragma unroll
        for (int it = 0; it < IPT; ++it)
            if ((uint64_t)it + my0 == t0 + tlen - 1) s_carry = key[it];
        uint32_t nh, wtile;
        uint32_t u = block_excl_sum<uint32_t>((uint32_t)__popc(heads), s_tmp, &nh);
        uint32_t wpre = block_excl_sum<uint32_t>(wsum, s_tmp, &wtile);  // the tile's weight before this thread's keys
        const uint64_t ubase = s_state[0];
        const uint64_t open_head = s_state[1];
        const uint64_t w0 = s_state[2];
        const uint32_t u0 = u;
#pragma unroll
        for (int it = 0; it < IPT; ++it) {
            if ((heads >> it) & 1u) s_cnt[u++] = wpre;
            wpre += wt[it];
        }
        if (threadIdx.x == 0) s_cnt[nh] = wtile;
        __syncthreads();
        if (nh > 0 && threadIdx.x == 0 && open_head != ~0ull)  // close the run left open by the previous tile
            out_counts[b.begin + ubase - 1] = (uint32_t)(w0 + s_cnt[0] - open_head);
        u = u0;
#pragma unroll
        for (int it = 0; it < IPT; ++it) {
            if ((heads >> it) & 1u) {
                store_key(out_keys, b.begin + ubase + u, key[it] & kmask);
                if (u + 1 < nh) out_counts[b.begin + ubase + u] = s_cnt[u + 1] - s_cnt[u];
                ++u;
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            if (nh > 0) {
                s_state[0] = ubase + nh;
                s_state[1] = w0 + s_cnt[nh - 1];
            }
            s_state[2] = w0 + wtile;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const uint64_t ub = s_state[0];
        if (ub > 0) out_counts[b.begin + ub - 1] = (uint32_t)(s_state[2] - s_state[1]);
        bucket_unique[qi] = ub;
    }
}

hipError_t launch_bucket_sort_large(int KW, const BucketSrc &src, const Bucket *buckets, uint64_t nbuckets, int k,
                                    uint64_t *scratch, uint64_t *out_keys, uint32_t *out_counts,
                                    uint64_t *bucket_unique, const uint32_t *list, hipStream_t s,
                                    unsigned long long *scratch_cursor) {
    if (!nbuckets) return hipSuccess;
    if (KW == 1)
        k_bucket_sort_large<1><<<(unsigned)nbuckets, NT, 0, s>>>(src, buckets, k, scratch, out_keys, out_counts,
                                                                   bucket_unique, list, scratch_cursor);
    else
        k_bucket_sort_large<2><<<(unsigned)nbuckets, NT, 0, s>>>(src, buckets, k, scratch, out_keys, out_counts,
                                                                   bucket_unique, list, scratch_cursor);
    return hipGetLastError();
}

