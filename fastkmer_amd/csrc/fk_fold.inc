// fk_fold.inc: the fold of a staged piece's duplicate k-mers into weighted keys -- included by
// fk_kernels.hip inside namespace fk, after fk_count_sorted.inc (WKeySpec, EMPTY_KEY).
// ---------------------------------------------------------------------------
// A job's count reads every k-mer of every staged piece after the last input byte has landed, and a
// read set's k-mers repeat (configs[1]: 4.7 occurrences per distinct k-mer).  A piece that landed
// earlier is folded while the rest of the input is still on the wire: per super-cell, its keys are
// deduplicated in an LDS table and written back as weighted keys (weight <= wmax in the four bits
// above the k-mer; a k-mer seen m times yields ceil(m / wmax) entries), cell by cell, so the piece
// keeps its format -- a key array laid out by cell and the cells' exclusive scan -- with fewer keys.
//   k_fold_sc      one workgroup per (bin, super-cell): its cells in batches of at most FOLD_HC keys
//                  (consecutive cells packed greedily; a larger cell is copied through unfolded), each
//                  batch deduplicated, its entries counting-sorted by cell and written to `mid` behind
//                  the previous batch's, from the super-cell's raw offset on; fcount = entries per cell
//   (scan of fcount: the piece's new cell offsets)
//   k_fold_compact each super-cell's run from `mid` to its dense place in the piece's key array; the
//                  job's cell totals take the folded counts
// ---------------------------------------------------------------------------

constexpr uint32_t FOLD_HS = 2 * FOLD_HC;    // table slots (load <= 1/2)
constexpr int FOLD_KPT = FOLD_HC / NT;       // keys per thread and batch
constexpr int FOLD_SPT = FOLD_HS / NT;       // slots per thread
constexpr uint32_t FOLD_MAXC = 64;           // cells per super-cell at most (F2 <= 6)
static_assert((FOLD_HS & (FOLD_HS - 1)) == 0 && FOLD_HC % NT == 0 && FOLD_MAXC <= NT, "fold table");

// SAMPLE: count only -- super-cell blockIdx.x * stride, nothing written but io[0] += keys read,
// io[1] += the entries they fold to
template <bool SAMPLE>
__global__ __launch_bounds__(NT) void k_fold_sc(const uint64_t *__restrict__ keys, const uint64_t *__restrict__ cb,
                                                uint64_t nsc, int k, int F, int F2, uint32_t wmax, uint32_t stride,
                                                uint64_t *__restrict__ mid, uint32_t *__restrict__ fcount,
                                                unsigned long long *io) {
    __shared__ unsigned long long s_k[FOLD_HS];
    __shared__ uint32_t s_c[FOLD_HS];
    __shared__ uint64_t s_cb[FOLD_MAXC + 1];
    __shared__ uint32_t s_cc[FOLD_MAXC], s_cp[FOLD_MAXC];  // entries per cell of the batch, their cursors
    __shared__ uint32_t s_tot;
    const uint32_t tid = threadIdx.x;
    const uint64_t sc = (uint64_t)blockIdx.x * stride;
    if (sc >= nsc) return;
    const uint32_t ncs = 1u << F2;  // cells per super-cell
    const uint64_t g0 = sc << F2;
    if (tid <= ncs) s_cb[tid] = cb[g0 + tid];
    __syncthreads();
    const WKeySpec ws = wkey_spec(k);
    const int sh = 2 * k - F;
    uint64_t cursor = s_cb[0];  // the next batch's entries go here
    unsigned long long tin = 0, tout = 0;
    for (uint32_t c = 0; c < ncs;) {  // uniform
        // the batch: cells [c, e) of at most FOLD_HC keys together, or one larger cell
        // (a lane per cell: the cells from c on whose end still fits are a prefix -- one ballot, not
        // a chain of dependent LDS reads)
        const uint64_t b0 = s_cb[c];
        const uint32_t lane = tid & 63u;
        const bool fits = lane >= c && lane < ncs && s_cb[lane + 1] - b0 <= FOLD_HC;
        const uint64_t fm = __ballot(fits) >> c;
        const uint32_t run = ~fm ? (uint32_t)__builtin_ctzll(~fm) : 64u;
        const uint32_t e = c + (run ? run : 1u);
        const uint64_t nb = s_cb[e] - b0;
        if (nb > FOLD_HC || nb == 0) {  // uniform: one cell copied through, or empty cells
            if constexpr (!SAMPLE) {
                for (uint64_t i = tid; i < nb; i += NT) mid[cursor + i] = keys[b0 + i];
                if (tid >= c && tid < e) fcount[g0 + tid] = (uint32_t)(s_cb[tid + 1] - s_cb[tid]);
            }
            tin += nb, tout += nb, cursor += nb;
            c = e;
            continue;
        }
        for (uint32_t s = tid; s < FOLD_HS; s += NT) s_k[s] = EMPTY_KEY, s_c[s] = 0;
        if (tid < FOLD_MAXC) s_cc[tid] = 0;
        __syncthreads();
        // 1. dedupe: the batch's keys loaded together, then inserted (weights added)
        uint64_t x[FOLD_KPT];
#pragma unroll
        for (int q = 0; q < FOLD_KPT; ++q) {
            const uint32_t i = q * NT + tid;
            x[q] = i < nb ? keys[b0 + i] : EMPTY_KEY;
        }
#pragma unroll
        for (int q = 0; q < FOLD_KPT; ++q) {
            if (x[q] == EMPTY_KEY) continue;
            uint32_t wt;
            const uint64_t key = wkey_split(x[q], ws, wt);
            uint32_t s = (uint32_t)((key * 0x9e3779b97f4a7c15ull) >> (64 - __builtin_ctz(FOLD_HS)));
            for (;;) {
                unsigned long long cur = s_k[s];
                if (cur == EMPTY_KEY) cur = atomicCAS(&s_k[s], EMPTY_KEY, (unsigned long long)key);
                if (cur == EMPTY_KEY || cur == key) {
                    atomicAdd(&s_c[s], wt);
                    break;
                }
                s = (s + 1) & (FOLD_HS - 1);
            }
        }
        __syncthreads();
        // 2. entries per cell: a k-mer of multiplicity m takes ceil(m / wmax)
#pragma unroll
        for (int q = 0; q < FOLD_SPT; ++q) {
            const uint32_t s = q * NT + tid;
            const unsigned long long key = s_k[s];
            if (key != EMPTY_KEY) atomicAdd(&s_cc[(uint32_t)(key >> sh) & (ncs - 1)], (s_c[s] + wmax - 1) / wmax);
        }
        __syncthreads();
        if (tid < 64) {  // wave 0: the cells' offsets in the batch
            const uint32_t v = tid < ncs ? s_cc[tid] : 0u;
            const uint32_t inc = wave_incl_sum<uint32_t>(v);
            s_cp[tid] = inc - v;
            if (tid == 63) s_tot = inc;
            if constexpr (!SAMPLE)
                if (tid >= c && tid < e) fcount[g0 + tid] = v;
        }
        __syncthreads();
        const uint32_t btot = s_tot;  // <= nb: an entry stands for at least one key
        // 3. the entries, by cell (order inside a cell is irrelevant)
        if constexpr (!SAMPLE) {
#pragma unroll
            for (int q = 0; q < FOLD_SPT; ++q) {
                const uint32_t s = q * NT + tid;
                const unsigned long long key = s_k[s];
                if (key == EMPTY_KEY) continue;
                const uint32_t m = s_c[s], ne = (m + wmax - 1) / wmax;
                const uint64_t at = cursor + atomicAdd(&s_cp[(uint32_t)(key >> sh) & (ncs - 1)], ne);
                for (uint32_t t = 0; t < ne; ++t) {
                    const uint32_t w = t + 1 < ne ? wmax : m - (ne - 1) * wmax;
                    mid[at + t] = key | ((uint64_t)(w - 1) << ws.wsh);
                }
            }
        }
        tin += nb, tout += btot, cursor += btot;
        c = e;
        __syncthreads();  // the table and the cell counters are reused
    }
    if constexpr (SAMPLE) {
        if (tid == 0) {
            atomicAdd(&io[0], tin);
            atomicAdd(&io[1], tout);
        }
    }
}

__global__ __launch_bounds__(NT) void k_fold_compact(const uint64_t *__restrict__ mid,
                                                     const uint64_t *__restrict__ cb_raw,
                                                     const uint64_t *__restrict__ cb_new,
                                                     const uint32_t *__restrict__ fcount, int F2,
                                                     uint64_t *__restrict__ keys, uint64_t *__restrict__ total) {
    const uint32_t ncs = 1u << F2;
    const uint64_t g0 = (uint64_t)blockIdx.x << F2;
    const uint64_t src = cb_raw[g0], dst = cb_new[g0], n = cb_new[g0 + ncs] - dst;
    for (uint64_t i = threadIdx.x; i < n; i += NT) keys[dst + i] = mid[src + i];
    if (threadIdx.x < ncs) {
        const uint64_t g = g0 + threadIdx.x;
        total[g] -= (cb_raw[g + 1] - cb_raw[g]) - fcount[g];
    }
}

hipError_t launch_fold_sc(const uint64_t *keys, const uint64_t *cb, uint32_t nlbins, int k, int F, int F2,
                          uint32_t wmax, uint64_t *mid, uint32_t *fcount, hipStream_t s) {
    const uint64_t nsc = (uint64_t)nlbins << (F - F2);
    if (!nsc) return hipSuccess;
    if (F2 > 6 || 2 * k > WKEY_MAX_BITS || wmax < 1 || wmax > WKEY_WMAX || nsc > 0x7fffffffull) return hipErrorInvalidValue;
    k_fold_sc<false><<<(unsigned)nsc, NT, 0, s>>>(keys, cb, nsc, k, F, F2, wmax, 1u, mid, fcount, nullptr);
    return hipGetLastError();
}

hipError_t launch_fold_sample(const uint64_t *keys, const uint64_t *cb, uint32_t nlbins, int k, int F, int F2,
                              uint32_t wmax, uint32_t stride, unsigned long long *io, hipStream_t s) {
    const uint64_t nsc = (uint64_t)nlbins << (F - F2);
    if (!nsc) return hipSuccess;
    if (F2 > 6 || 2 * k > WKEY_MAX_BITS || wmax < 1 || wmax > WKEY_WMAX || !stride || nsc > 0x7fffffffull)
        return hipErrorInvalidValue;
    k_fold_sc<true><<<(unsigned)((nsc + stride - 1) / stride), NT, 0, s>>>(keys, cb, nsc, k, F, F2, wmax, stride, nullptr,
                                                                          nullptr, io);
    return hipGetLastError();
}

hipError_t launch_fold_compact(const uint64_t *mid, const uint64_t *cb_raw, const uint64_t *cb_new,
                               const uint32_t *fcount, uint32_t nlbins, int F, int F2, uint64_t *keys,
                               uint64_t *total, hipStream_t s) {
    const uint64_t nsc = (uint64_t)nlbins << (F - F2);
    if (!nsc) return hipSuccess;
    if (F2 > 6 || nsc > 0x7fffffffull) return hipErrorInvalidValue;
    k_fold_compact<<<(unsigned)nsc, NT, 0, s>>>(mid, cb_raw, cb_new, fcount, F2, keys, total);
    return hipGetLastError();
}
