// fk_fastq.inc: FASTQ records to FASTA byte classes, in place -- included by fk_kernels.hip inside namespace fk.
// ---------------------------------------------------------------------------
// 0. FASTQ normalisation (in front of stage 1; the parse kernels keep one grammar)
//
// Strict four-line records: "@name", sequence, "+[anything]", quality.  The
// stage turns a record-aligned byte range [a, b) of the device input into
// text the FASTA parsers read as the same reads: the '@', the '+' and the
// first byte of a non-empty quality line become '>', so the '+' and quality
// lines are header lines to them.  No newline moves and no offset changes.
// With min_q > 0 every sequence byte whose quality is below it becomes 'N'.
//
// Two kernels over the range:
//   k_fq_lines    reads the range once (SWAR byte tests, 64 bytes a thread) and
//                 compacts the offsets of its newlines into an index (4 B a
//                 line, range-relative) with a block scan and the decoupled
//                 look-back; it also notes, per tile, the last byte that is
//                 neither '\n' nor '\r' (the trailing blank lines of the input's
//                 end lie behind the last of them; one word a tile, no shared
//                 atomic) and, for a borrowed input, writes the copy the stage
//                 works on.
//   k_fq_records  runs per record off the index, a wave per 64 records: one
//                 lane a record checks the '@', the '+' and the two lengths;
//                 the wave walks each record's quality line (64 bytes a step);
//                 one lane a record writes the three marks.  Grid-strided over
//                 the record count, which only the device knows.
// Malformed records raise info[2]; counts go to info[0] (records) and info[1]
// (masked bases).  The host reads info with the map's counters.
// ---------------------------------------------------------------------------

constexpr int FQ_NT = 256;
constexpr int FQ_TILE = FQ_NT * 64;  // bytes per k_fq_lines workgroup (64 per thread)

struct FqMeta {          // per launch pair; zeroed by the host
    uint32_t n_nl;       // newlines in the range
    uint32_t pad0;
    uint64_t rec_base;   // records of the job before this range
    uint32_t pad[12];
};
static_assert(sizeof(FqMeta) == 64, "FqMeta is the first 64 bytes of the workspace");

__global__ __launch_bounds__(FQ_NT) void k_fq_lines(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
                                                    uint64_t a, uint64_t b, uint64_t *status, uint32_t *tile_text,
                                                    uint32_t *nl_idx, uint32_t cap, FqMeta *meta,
                                                    unsigned long long *info) {
    __shared__ uint32_t s_tmp[FQ_NT / 64], s_text[FQ_NT / 64];
    __shared__ uint32_t s_base;
    const int tid = threadIdx.x;
    const uint64_t tile = blockIdx.x;
    const uint64_t a0 = a & ~63ull;  // threads own 64-byte aligned chunks of the buffer
    const uint64_t p0 = a0 + tile * FQ_TILE + (uint64_t)tid * 64;

    uint32_t w[16];
    load64(src, b, p0, w);
    const int hi = p0 >= b ? 0 : (int)min<uint64_t>(64, b - p0);
    const int lo = p0 >= a ? 0 : (int)min<uint64_t>(64, a - p0);
    const uint64_t inr = low_mask(hi) & ~low_mask(lo);
    uint64_t nl = 0, cr = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        nl |= (uint64_t)zero_bytes4(w[i] ^ 0x0a0a0a0au) << (4 * i);
        cr |= (uint64_t)zero_bytes4(w[i] ^ 0x0d0d0d0du) << (4 * i);
    }
    const uint64_t text = ~(nl | cr) & inr;
    nl &= inr;

    if (dst) {  // the copy of a borrowed input
        if (inr == ~0ull && ((reinterpret_cast<uintptr_t>(dst + p0) & 15) == 0)) {
            typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
            u32x4 *d = reinterpret_cast<u32x4 *>(dst + p0);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                u32x4 q;
                q.x = w[4 * i + 0], q.y = w[4 * i + 1], q.z = w[4 * i + 2], q.w = w[4 * i + 3];
                d[i] = q;
            }
        } else {
            for (int j = lo; j < hi; ++j) dst[p0 + j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
        }
    }

    // the tile's last text byte: 1 + its range offset, 0 for a tile of blank lines
    const uint32_t my_text = text ? (uint32_t)(p0 + 63 - __clzll(text) - a) + 1u : 0u;
    const uint32_t wave_text = wave_incl_max<uint32_t>(my_text);
    if ((tid & 63) == 63) s_text[tid >> 6] = wave_text;

    uint32_t tile_n;
    const uint32_t my_off = block_excl_sum<uint32_t, true, FQ_NT>((uint32_t)__popcll(nl), s_tmp, &tile_n);
    if (tid == FQ_NT - 1) {
        uint32_t t = 0;
#pragma unroll
        for (int w = 0; w < FQ_NT / 64; ++w) t = max(t, s_text[w]);
        tile_text[tile] = t;
    }
    if (tid < 64) {
        const uint64_t ex = lookback_excl(status, tile, tile_n, LbSum());
        if (tid == 0) {
            s_base = (uint32_t)ex;
            if (tile == gridDim.x - 1) {
                meta->n_nl = (uint32_t)ex + tile_n;
                meta->rec_base = info[0];
            }
        }
    }
    __syncthreads();
    uint32_t idx = s_base + my_off;
    bool over = false;
    while (nl) {
        const int bit = __builtin_ctzll(nl);
        nl &= nl - 1;
        if (idx < cap)
            nl_idx[idx] = (uint32_t)(p0 + bit - a);
        else
            over = true;
        ++idx;
    }
    if (over) atomicOr(&info[3], 1ull);
}

// lines of the range: line i spans [fq_start(i), fq_end(i)) without its '\n'
__device__ __forceinline__ uint32_t fq_start(const uint32_t *nl_idx, uint32_t i) { return i ? nl_idx[i - 1] + 1u : 0u; }
__device__ __forceinline__ uint32_t fq_end(const uint32_t *nl_idx, uint32_t nnl, uint32_t len, uint32_t i) {
    return i < nnl ? nl_idx[i] : len;
}

__global__ __launch_bounds__(FQ_NT) void k_fq_records(uint8_t *fa, uint64_t a, uint64_t b, const uint32_t *nl_idx,
                                                      uint32_t cap, const FqMeta *meta, const uint32_t *tile_text,
                                                      uint32_t ntiles, int final_, int min_q, int q_off,
                                                      unsigned long long *info) {
    __shared__ uint32_t s_nrec;
    const int tid = threadIdx.x, lane = tid & 63;
    const uint32_t nnl = meta->n_nl;
    if (nnl > cap) return;  // the index overflowed (info[3] is set): nothing is touched
    const uint32_t len = (uint32_t)(b - a);
    const uint64_t rec_base = meta->rec_base;
    if (tid == 0) {
        // lines that count: all of a range inside the input (it ends at a record start); at the
        // input's end the lines up to the last text byte, rounded up to a whole record where blank
        // lines follow (an empty quality line is a blank line too)
        const uint32_t nlines = nnl + ((len && (nnl == 0 || nl_idx[nnl - 1] + 1u < len)) ? 1u : 0u);
        uint32_t neff = final_ ? 0u : nnl;
        uint32_t last_text = 0;  // the last tile that holds text has the input's last text byte
        for (uint32_t t = ntiles; final_ && t-- > 0 && !last_text;) last_text = tile_text[t];
        if (final_ && last_text) {
            const uint32_t t = last_text - 1u;
            uint32_t lo = 0, hi = nnl;  // newlines before t
            while (lo < hi) {
                const uint32_t mid = lo + (hi - lo) / 2;
                if (nl_idx[mid] < t)
                    lo = mid + 1;
                else
                    hi = mid;
            }
            const uint32_t ntext = lo + 1u;
            neff = min(nlines, (ntext + 3u) & ~3u);
        }
        s_nrec = neff / 4u;
        if (blockIdx.x == 0) {
            // a range that does not end with a record: the input ends inside one, or a line is missing
            if (neff & 3u) atomicMax(&info[2], ~(rec_base + neff / 4u));
            if (neff / 4u) atomicAdd(&info[0], (unsigned long long)(neff / 4u));
        }
    }
    __syncthreads();
    const uint32_t nrec = s_nrec;
    uint8_t *f = fa + a;
    const uint32_t nwaves = gridDim.x * (FQ_NT / 64);
    uint32_t masked = 0;
    for (uint64_t base = ((uint64_t)blockIdx.x * (FQ_NT / 64) + (tid >> 6)) * 64; base < nrec;
         base += (uint64_t)nwaves * 64) {
        const uint32_t r = (uint32_t)base + lane;
        const bool act = r < nrec;
        uint32_t s0 = 0, s1 = 0, s2 = 0, s3 = 0, e3 = 0, len1 = 0, q0 = 0;
        bool ok = false;
        if (act) {
            const uint32_t i0 = 4u * r;
            s0 = fq_start(nl_idx, i0);
            const uint32_t e0 = nl_idx[i0];
            s1 = e0 + 1u;
            const uint32_t e1 = nl_idx[i0 + 1];
            s2 = e1 + 1u;
            const uint32_t e2 = nl_idx[i0 + 2];
            s3 = e2 + 1u;
            e3 = fq_end(nl_idx, nnl, len, i0 + 3);
            len1 = e1 - s1;
            if (len1 && f[e1 - 1] == '\r') --len1;
            uint32_t len3 = e3 - s3;
            if (len3 && f[e3 - 1] == '\r') --len3;
            ok = e0 > s0 && f[s0] == '@' && e2 > s2 && f[s2] == '+' && len1 == len3;
            if (!ok) atomicMax(&info[2], ~(rec_base + r));
            q0 = len3 ? f[s3] : 0u;
        }
        if (min_q > 0) {
            // the quality is read before the line's first byte is marked below (and that byte by its
            // record's own lane, above)
            const int nj = (int)min<uint64_t>(64, nrec - base);
            for (int j = 0; j < nj; ++j) {
                const bool okj = __shfl((int)ok, j, 64) != 0;
                const uint32_t n1 = __shfl(len1, j, 64), sq = __shfl(s1, j, 64), qq = __shfl(s3, j, 64);
                const uint32_t qj = __shfl(q0, j, 64);
                if (!okj) continue;
                for (uint32_t t = lane; t < n1; t += 64) {
                    const int q = t ? (int)f[qq + t] : (int)qj;
                    if (q - q_off < min_q) {
                        f[sq + t] = 'N';
                        ++masked;
                    }
                }
            }
        }
        if (act && ok) {
            f[s0] = '>';
            f[s2] = '>';
            if (e3 > s3) f[s3] = '>';
        }
    }
    if (min_q > 0) {
        const uint32_t wm = wave_incl_sum<uint32_t>(masked);
        if (lane == 63 && wm) atomicAdd(&info[1], (unsigned long long)wm);
    }
}

// Workspace of one normalise launch over `range` bytes: FqMeta, the look-back status words, a word
// per tile for its last text byte, the newline index (one entry per 4 bytes and 4096 more: an input with more lines raises info[3]).
static uint64_t fq_tiles(uint64_t range) { return (range + 63 + FQ_TILE - 1) / FQ_TILE; }
static uint64_t fq_cap(uint64_t range) { return std::min<uint64_t>(range / 4 + 4096, 0xffffffffull); }
uint64_t fastq_ws_bytes(uint64_t range) { return sizeof(FqMeta) + fq_tiles(range) * 12 + 128 + fq_cap(range) * 4; }

// Normalises [a, b) of buf (b - a < 2^32); src != nullptr: the bytes are first copied from
// src[a, b) (same offsets).  final_: the input ends at b.  info: the job's four counters.
hipError_t launch_fastq_normalise(uint8_t *buf, const uint8_t *src, uint64_t a, uint64_t b, int final_, int min_q,
                                  int q_off, void *ws, unsigned long long *info, hipStream_t s) {
    if (b <= a) return hipSuccess;
    const uint64_t range = b - a, a0 = a & ~63ull;
    const uint64_t ntiles = (b - a0 + FQ_TILE - 1) / FQ_TILE;
    const uint32_t cap = (uint32_t)fq_cap(range);
    FqMeta *meta = (FqMeta *)ws;
    uint64_t *status = (uint64_t *)((char *)ws + sizeof(FqMeta));
    const uint64_t st_bytes = (fq_tiles(range) * 8 + 63) & ~63ull, tt_bytes = (fq_tiles(range) * 4 + 63) & ~63ull;
    uint32_t *tile_text = (uint32_t *)((char *)ws + sizeof(FqMeta) + st_bytes);
    uint32_t *nl_idx = (uint32_t *)((char *)ws + sizeof(FqMeta) + st_bytes + tt_bytes);
    hipError_t e = hipMemsetAsync(ws, 0, sizeof(FqMeta) + ntiles * 8, s);
    if (e != hipSuccess) return e;
    k_fq_lines<<<(unsigned)ntiles, FQ_NT, 0, s>>>(src ? src : buf, src ? buf : nullptr, a, b, status, tile_text, nl_idx,
                                                  cap, meta, info);
    const unsigned nb = (unsigned)std::clamp<uint64_t>(range / 16384, 1, 2048);
    k_fq_records<<<nb, FQ_NT, 0, s>>>(buf, a, b, nl_idx, cap, meta, tile_text, (uint32_t)ntiles, final_, min_q, q_off,
                                      info);
    return hipGetLastError();
}
