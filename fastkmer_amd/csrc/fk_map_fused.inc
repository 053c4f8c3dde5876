// fk_map_fused.inc: stages 1 + 2 in one kernel -- FASTA bytes to super-k-mer
// records (FASTdoop record reader + getSuperKmers, SBKC:62-65, :34-169) --
// included by fk_kernels.hip inside namespace fk, after fk_parse.inc and
// fk_signature.inc (whose byte classes, norm blocks and record cuts it uses).
// ---------------------------------------------------------------------------
// A workgroup of NTH threads parses NTH * 64 FASTA bytes starting at its tile
// t0 = tile * TILE, TILE = (NTH - FM_HALO_T) * 64: the last FM_HALO_T threads
// parse the first bytes of the next tile (the halo), so that every window that
// starts in the tile finds its k - 1 following positions in this workgroup's
// LDS.  Nothing between the FASTA and the records touches HBM:
//  1. byte classes (SWAR, as k_fasta_parse), the line state at the tile start
//     from a read-back of at most FM_SCAN_BYTES before t0, the line state of
//     every thread from one block max-scan over "last newline | header bit"
//     (no per-thread global byte loads), header / junk / newline removal;
//  2. compaction of the kept bytes into tile-local 2-bit codes and valid bits
//     in LDS (MSB-first, the layout k_superkmers reads from HBM);
//  3. the signature passes of k_superkmers over the tile's positions, one wave
//     per pass (no workgroup barrier); each pass stores a compact record per
//     super-k-mer into the tile's slots -- its header word (bin, n - 1, fine
//     hash) and its first position in the tile's code stream -- and the
//     workgroup stores the tile's code stream once (0.25 B per base): no
//     cross-tile dependency, so tiles never wait on each other.  The partition
//     builds the W-word records from the slots and the stream (RecSrc,
//     fk_partition.inc), so the map writes ~0.6 B per FASTA byte instead of the
//     ~1.8 B of whole 16-B records.
// Inputs the fast path cannot place -- a line longer than the read-back, text
// before the first header beyond tile 0, a halo with fewer than k - 1
// positions, more than FM_TCAP records in a tile -- raise counters[2]; the
// host then maps the input with the two-kernel path (k_fasta_parse +
// k_superkmers), which handles every input.  Tiles are independent, so the
// input can be mapped in consecutive launches (tile_begin) while later bytes
// are still in flight over PCIe (fk_ingest).
// ---------------------------------------------------------------------------

constexpr int FM_HALO_T = 4;           // threads parsing the next tile's first bytes
constexpr int FM_SCAN_BYTES = 4096;    // read-back for the line holding the tile start
constexpr int FM_LS_BIAS = FM_SCAN_BYTES + 1;  // tile-relative line starts + bias > 0
constexpr int FM_TCAP = 5120;          // record slots per tile (~2860 used at 100 bp reads)
constexpr int FM_CSLOT = 512 * 64 / 16 + 72;  // code-stream words per tile (FmGeom<512>::CODE_WORDS)
constexpr int FM_QCAP = 128;           // record starts per wave queued at a time
constexpr int FM_VSLOT = 512 * 64 / 32 + 40 + 4;  // split map: per tile (P_own, P_all, -, -, FmGeom<512>::VALID_WORDS valid words)
// fallback reasons (counters[2] bits, fk_stats.fused_fallback)
constexpr uint32_t FM_FB_LINE = 1;  // no newline within FM_SCAN_BYTES before a tile start
constexpr uint32_t FM_FB_JUNK = 2;  // the input does not start with '>' (text before the first header)
constexpr uint32_t FM_FB_HALO = 4;  // an owned window runs past the parsed halo
constexpr uint32_t FM_FB_DESC = 8;  // more than FM_TCAP records in a tile

#ifdef FK_PROBES
// measurement build only: per-phase wave cycles of k_map_fused (s_memtime stamps accumulated per
// wave in registers, added by lane 0 of each wave at the kernel's end into one of 64 slot rows --
// blockIdx % 64 -- so that the atomics do not serialize on one address); read with
// fk_debug_map_cycles (the rows summed)
constexpr int FM_CYC_ROWS = 64;
__device__ unsigned long long g_fm_cycles[FM_CYC_ROWS * 16];
__device__ __forceinline__ unsigned long long fm_stamp() {
    unsigned long long t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    __builtin_amdgcn_sched_barrier(0);
    return t;
}
#define FM_STAMP(i)                         \
    do {                                    \
        const unsigned long long t_ = fm_stamp(); \
        fm_acc[(i)] += t_ - fm_t0;          \
        fm_t0 = t_;                         \
    } while (0)
#define FM_FLUSH()                                                                                  \
    do {                                                                                            \
        if ((threadIdx.x & 63) == 0)                                                                \
            for (int i_ = 0; i_ < 9; ++i_)                                                          \
                atomicAdd(&g_fm_cycles[(blockIdx.x % FM_CYC_ROWS) * 16 + i_], fm_acc[i_]);          \
    } while (0)
#else
#define FM_STAMP(i) \
    do {            \
    } while (0)
#define FM_FLUSH() \
    do {           \
    } while (0)
#endif

template <int NTH>
struct FmGeom {
    static constexpr int TILE = (NTH - FM_HALO_T) * 64;      // owned bytes per tile
    static constexpr int SPAN = NTH * 64;                     // parsed bytes per tile
    // the last pass of a tile reads up to 64 lanes x 16 positions past its base (zeros)
    static constexpr int CODE_WORDS = SPAN / 16 + 72;
    static constexpr int VALID_WORDS = SPAN / 32 + 40;
};

constexpr int FM_NT = 512;  // threads per tile (256-thread tiles measured 2.5 vs 1.1 ms per GB)
uint64_t fm_tile_bytes(int nth) { return nth == FM_NT ? FmGeom<FM_NT>::TILE : 0; }
uint64_t fm_span_bytes(int nth) { return nth == FM_NT ? FmGeom<FM_NT>::SPAN : 0; }

// Compaction of one 32-byte half: the kept bytes' 2-bit codes (C, byte i at bits 2i) and valid
// bits (V) are appended run by run to acc / vacc, na counting the appended positions.
__device__ __forceinline__ void fm_compact32(uint32_t K, uint64_t C, uint32_t V, uint64_t &acc, uint32_t &vacc,
                                             int &na) {
    while (K) {
        const int s = __builtin_ctz(K);
        const uint32_t rest = ~(K >> s);
        const int len = rest ? __builtin_ctz(rest) : 32;  // len + s <= 32
        const uint64_t bits = (C >> (2 * s)) & (~0ull >> (64 - 2 * len));
        acc |= bits << (2 * na);  // na + len <= 32
        const uint32_t lm = len >= 32 ? ~0u : ((1u << len) - 1u);
        vacc |= ((V >> s) & lm) << na;
        na += len;
        K &= ~(lm << s);
    }
}

// DPP lane move that reads 0 for lanes without a source (bound_ctrl): no identity register, and
// an add / max of its result fuses into one DPP instruction
template <int CTRL, int ROWM = 0xf>
__device__ __forceinline__ uint32_t dppz(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROWM, 0xf, true);
}
// inclusive wave sum: six DPP adds (the compiler keeps each hop a separate move); s_nop 1 before
// each, the VALU-write -> DPP-read wait states
__device__ __forceinline__ uint32_t wave_incl_sum_z(uint32_t v) {
    asm volatile(
        "s_nop 1\n\tv_add_u32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "s_nop 1\n\tv_add_u32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "s_nop 1\n\tv_add_u32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "s_nop 1\n\tv_add_u32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "s_nop 1\n\tv_add_u32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
        "s_nop 1\n\tv_add_u32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
        "s_nop 1"
        : "+v"(v));
    return v;
}

// ~(x & mask) & a in one v_bitop3 (the compiler turns `& a` of a sign-extended bit into a compare
// and a select); truth-table index = x << 2 | mask << 1 | a
__device__ __forceinline__ uint32_t fm_nand_and(uint32_t x, uint32_t mask, uint32_t a) {
    uint32_t r;
    asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0x2a" : "=v"(r) : "v"(x), "s"(mask), "v"(a));
    return r;
}

// norms of the 16 m-mers starting at 16 * blk (bases 16 blk .. 16 blk + 30), as norm_block<false>
// (fk_signature.inc) with 32-bit bit-field extracts: the forward m-mers from the 16-base words
// starting at multiples of D = 17 - m, the reverse complements likewise from the reversed
// window, and the forbidden flags as sign-extended one-bit fields ORed in (all ones: never the
// minimum below 4^m).
template <int MC, bool INV = false>
__device__ __forceinline__ void fm_norm_block(const uint32_t *s_codes, int blk, uint32_t out[16]) {
    constexpr int m = MC, D = 17 - MC;
    const uint32_t hi = s_codes[blk], lo = s_codes[blk + 1];
    const uint64_t win = ((uint64_t)hi << 32) | lo;
    const uint64_t rw = revcomp64(win, 32);  // base 31 - j of the window at bits 2j (LSB-first)
    const uint32_t rlo = (uint32_t)rw, rhi = (uint32_t)(rw >> 32);
    constexpr uint64_t E = 0x5555555555555555ull;
    const uint64_t h1 = win >> 1;
    const uint64_t isA = ~(win | h1) & E, isT = win & h1 & E;
    const uint64_t isC = win & ~h1 & E, isG = h1 & ~win & E;
    const uint32_t fF = (uint32_t)((or_run(isA & (isA << 2), m - 1) | (isA & (isC << 2) & (isA << 4))) >> 32);
    const uint32_t fR =
        (uint32_t)((or_run(isT & (isT << 2), m - 1) | ((isT & (isG << 2) & (isT << 4)) << (2 * (m - 3)))) >> 32);
    constexpr uint32_t def = 1u << (2 * m), M = def - 1u;
    // INV: the bitwise complement of the norm (the window minimum becomes a maximum, whose identity
    // 0 is what DPP lane shifts with bound_ctrl read for lanes without a source): per strand
    // ~(m-mer) & (all ones if allowed, else 0) -- ~((w >> o) & M) & a, one 3-input bit op -- and the
    // maximum with ~4^m
    const uint32_t aF = ~fF, aR = ~fR;  // allowed flags
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        const int a = (s / D) * D;  // the m-mer lies in bases a .. a + 15
        const uint32_t fw = a == 0 ? hi : __builtin_amdgcn_alignbit(hi, lo, 32 - 2 * a);
        const uint32_t rv = a == 0 ? rlo : __builtin_amdgcn_alignbit(rhi, rlo, 2 * a);
        if constexpr (INV) {
            const uint32_t af = (uint32_t)__builtin_amdgcn_sbfe((int)aF, 30 - 2 * s, 1);
            const uint32_t ar = (uint32_t)__builtin_amdgcn_sbfe((int)aR, 30 - 2 * s, 1);
            const uint32_t tf = fm_nand_and(fw >> (2 * (16 - (s - a) - m)), M, af);
            const uint32_t tr = fm_nand_and(rv >> (2 * (s - a)), M, ar);
            out[s] = max(max(tf, tr), ~def);
        } else {
            const uint32_t v = __builtin_amdgcn_ubfe(fw, 2 * (16 - (s - a) - m), 2 * m);
            const uint32_t r = __builtin_amdgcn_ubfe(rv, 2 * (s - a), 2 * m);
            const uint32_t xf = (uint32_t)__builtin_amdgcn_sbfe((int)fF, 30 - 2 * s, 1);
            const uint32_t xr = (uint32_t)__builtin_amdgcn_sbfe((int)fR, 30 - 2 * s, 1);
            out[s] = min(min(v | xf, r | xr), def);
        }
    }
}

// acc * 2 + (a != b): the compare's lane mask is the carry-in of the add
__device__ __forceinline__ uint32_t fm_push_ne(uint32_t acc, uint32_t a, uint32_t b) {
    uint32_t r;
    asm("v_cmp_ne_u32 vcc, %1, %2\n\tv_addc_co_u32 %0, vcc, %3, %3, vcc" : "=v"(r) : "v"(a), "v"(b), "v"(acc)
                 : "vcc");
    return r;
}

// word index of element s of lane l in a wave's window-minimum scratch: 16 words per lane, the
// four 16-byte groups rotated by (l >> 2) & 3 so that a wave's 16-byte stores hit distinct banks
__device__ __forceinline__ uint32_t fm_scr(uint32_t l, uint32_t s) {
    return l * 16 + ((((s >> 2) ^ (l >> 2)) & 3u) << 2) + (s & 3u);
}

// per tile: tcnt = records, tstat = (k-mers, positions) (k_tile_totals sums them into counters[0],
// [1], [3]); counters[2]: fallback flags.  Record slot j of tile t: hdrs[t * FM_TCAP + j] = header
// word (bin | (n - 1) << 22 | fine << 26), pos[t * FM_TCAP + j] = its first position in the tile's
// code stream codes[t * FM_CSLOT ...] (16 bases per word, MSB-first)
template <int NTH, int KC, int MC, int MODE>
__global__ __launch_bounds__(NTH) void k_map_fused(const uint8_t *__restrict__ fa, uint64_t n, int more,
                                                   uint64_t tile_begin, FastMod fm, uint32_t *__restrict__ hdrs,
                                                   uint16_t *__restrict__ pos, uint32_t *__restrict__ codes,
                                                   uint32_t *__restrict__ tcnt, uint32_t *__restrict__ tstat,
                                                   uint32_t *__restrict__ vslots, unsigned long long *counters,
                                                   int probe) {
    using Gm = FmGeom<NTH>;
    static_assert(Gm::CODE_WORDS <= FM_CSLOT && Gm::SPAN <= 65536, "code slot / u16 positions");
    constexpr int k = KC, m = MC, w = KC - MC + 1;
    (void)m;
    static_assert(w >= 17, "the fused path uses the suffix-min window (k - m >= 16)");
    __shared__ uint32_t s_code[Gm::CODE_WORDS];
    __shared__ uint32_t s_valid[Gm::VALID_WORDS];
    __shared__ __attribute__((aligned(16))) uint32_t s_wscr[NTH / 64 * 1024];  // per wave: window minima of a pass
    __shared__ uint32_t s_wstop[NTH];                                        // per wave: stop masks of a pass
    __shared__ uint32_t s_wq[NTH / 64 * FM_QCAP];                            // per wave: queued record starts
    __shared__ int64_t s_tmp64[NTH / 64];
    __shared__ uint32_t s_tmp32[NTH / 64];
    __shared__ uint32_t s_sum[NTH / 64];
    __shared__ int s_tmpi[NTH / 64];
    __shared__ uint32_t s_wnk[NTH / 64], s_wovf, s_tcnt;
    __shared__ uint64_t s_bcast[2];
    __shared__ uint32_t s_pown, s_pall;

#ifdef FK_PROBES
    unsigned long long fm_t0 = fm_stamp(), fm_acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#endif
    const int tid = threadIdx.x;
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const bool fa16 = (reinterpret_cast<uintptr_t>(fa) & 15) == 0;
    auto load_rb = [&](uint64_t a, uint32_t (&w4)[4]) {
        if (fa16) {
            const u32x4 v = *reinterpret_cast<const u32x4 *>(fa + a);
            w4[0] = v.x, w4[1] = v.y, w4[2] = v.z, w4[3] = v.w;
        } else {
            for (int i = 0; i < 4; ++i)
                w4[i] = (uint32_t)fa[a + 4 * i] | ((uint32_t)fa[a + 4 * i + 1] << 8) |
                        ((uint32_t)fa[a + 4 * i + 2] << 16) | ((uint32_t)fa[a + 4 * i + 3] << 24);
        }
    };
    // The tile's input registers: the thread's 64 bytes; wave 0 also the first 1 KB read-back
    // window before the tile (line state, below), thread 0 the input's first byte and
    // the wave's last lane the first byte of the next thread's 64 (a line starting there is a
    // header iff it is '>'; the other lanes take it by a lane shift), all issued together so that
    // their latencies overlap
    uint32_t wv[16], rb0[4], fa_first, next_byte;
    auto tile_loads = [&](uint64_t tl) {
        const uint64_t t0_ = tl * (uint64_t)Gm::TILE, p0_ = t0_ + (uint64_t)tid * 64;

        load64(fa, n, p0_, wv);
        rb0[0] = rb0[1] = rb0[2] = rb0[3] = 0u;
        if (tid < 64 && t0_ >= 1024) load_rb(t0_ - 1024 + 16 * (uint64_t)tid, rb0);
        fa_first = (tid == 0 && t0_ > 0) ? (uint32_t)fa[0] : (uint32_t)'>';
        const bool last_lane = (tid & 63) == 63 && tid + 1 < NTH && p0_ + 64 < n;
        next_byte = last_lane ? (uint32_t)fa[p0_ + 64] : 0u;
    };
    {
    const uint64_t it = blockIdx.x;
    const uint64_t tile = tile_begin + it;
    const uint64_t t0 = tile * (uint64_t)Gm::TILE;
    uint32_t *const vs = vslots + it * (uint64_t)FM_VSLOT;  // MODE 1 / 2: this tile's (P_own, P_all, valid words)
    uint32_t P_own = 0, P_all = 0;
    if (tid == 0) s_wovf = 0u, s_tcnt = 0u;
    if constexpr (MODE == 2) {
        // the signature passes of the tiles MODE 1 parsed: their code and valid streams into LDS
        typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));
        const u32x4v *gc = reinterpret_cast<const u32x4v *>(codes + tile * (uint64_t)FM_CSLOT);
        const u32x4v *gv = reinterpret_cast<const u32x4v *>(vs);
        static_assert(Gm::CODE_WORDS % 4 == 0 && (Gm::VALID_WORDS + 4) % 4 == 0, "16-B rows");
        for (int i = tid; i < Gm::CODE_WORDS / 4; i += NTH) reinterpret_cast<u32x4v *>(s_code)[i] = gc[i];
        for (int i = tid; i < Gm::VALID_WORDS / 4 + 1; i += NTH) {
            const u32x4v v = gv[i];
            if (i == 0) {
                if (tid == 0) s_pown = v.x, s_pall = v.y;
            } else {
                reinterpret_cast<u32x4v *>(s_valid)[i - 1] = v;
            }
        }
        __syncthreads();
        P_own = s_pown, P_all = s_pall;
    } else {
    tile_loads(tile);
    const uint64_t p0 = t0 + (uint64_t)tid * 64;
    for (int i = tid; i < Gm::CODE_WORDS; i += NTH) s_code[i] = 0;
    for (int i = tid; i < Gm::VALID_WORDS; i += NTH) s_valid[i] = 0;

    // ---- 1. byte classes of this thread's 64 bytes (as k_fasta_parse)
#ifdef FK_PROBES
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    FM_STAMP(8);  // the tile's loads in flight (issue to the last byte landed)
#endif
    const int nb = p0 >= n ? 0 : (int)min<uint64_t>(64, n - p0);
    const uint64_t inr = low_mask(nb);
    uint32_t nlw[2] = {0u, 0u}, gtw[2] = {0u, 0u}, okw[2] = {0u, 0u}, cw[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 16; i += 2) {
        uint32_t zn[2], zg[2], zo[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const uint32_t x = wv[i + h];
            zn[h] = zero_bytes_msb(x ^ 0x0a0a0a0au);
            zg[h] = zero_bytes_msb(x ^ 0x3e3e3e3eu);
            const uint32_t c = ((x >> 1) ^ (x >> 2)) & 0x03030303u;          // A0 C1 G2 T3 (other bytes: any)
            const uint32_t e = __builtin_amdgcn_perm(0u, 0x54474341u, c);  // "ACGT"[c] per byte
            zo[h] = zero_bytes_msb(x ^ e);
            cw[(i + h) >> 2] |= __builtin_amdgcn_udot4(c, 0x40100401u, 0u, false) << (8 * ((i + h) & 3));
        }
        const int half = i >> 3, pos = 4 * (i & 7);
        const uint32_t dn =
            __builtin_amdgcn_udot4(zn[1], 0x80402010u, __builtin_amdgcn_udot4(zn[0], 0x08040201u, 0u, false), false);
        const uint32_t dg =
            __builtin_amdgcn_udot4(zg[1], 0x80402010u, __builtin_amdgcn_udot4(zg[0], 0x08040201u, 0u, false), false);
        const uint32_t dk =
            __builtin_amdgcn_udot4(zo[1], 0x80402010u, __builtin_amdgcn_udot4(zo[0], 0x08040201u, 0u, false), false);
        if (pos == 0) {
            nlw[half] |= dn >> 7;
            gtw[half] |= dg >> 7;
            okw[half] |= dk >> 7;
        } else {
            nlw[half] |= dn << (pos - 7);
            gtw[half] |= dg << (pos - 7);
            okw[half] |= dk << (pos - 7);
        }
    }
    const uint64_t nl = (((uint64_t)nlw[1] << 32) | nlw[0]) & inr;
    const uint64_t gt = (((uint64_t)gtw[1] << 32) | gtw[0]) & inr;
    const uint64_t ok = ((uint64_t)okw[1] << 32) | okw[0];
    const uint64_t clo = ((uint64_t)cw[1] << 32) | cw[0], chi = ((uint64_t)cw[3] << 32) | cw[2];
    FM_STAMP(0);  // loads + byte classes

    // ---- line state.  Per thread: (start of the line after its last newline) << 1 | that line is a
    // header ('>' first); the exclusive block max gives the line holding p0.  The tile's initial
    // value comes from reading back to the last newline before t0 (wave 0, 1 KB a step).
    // A line that starts at the next thread's first byte (newline at byte 63) is a header iff that
    // byte is '>': the lanes take their successor's first-byte class by a lane shift (the wave's last
    // lane from the byte it loaded).  Line starts are held
    // tile-relative (+ FM_LS_BIAS, so the read-back range stays positive) in 32-bit values; 0 = none.
    const uint32_t my_first = (uint32_t)(gt & 1ull);
    const uint32_t nxt_first = (tid & 63) == 63 ? (next_byte == '>' ? 1u : 0u)
                                                : dpp32<0x130, 0xf>(0u, my_first);  // wave_shl:1
    const uint32_t tile_first = (uint32_t)__builtin_amdgcn_readlane((int)my_first, 0);  // wave 0: thread 0
    uint32_t val = 0u;
    if (nl) {
        const int ql = 63 - __clzll(nl);
        const uint32_t hb = ql < 63 ? (uint32_t)(gt >> (ql + 1)) & 1u : nxt_first;
        val = ((uint32_t)(tid * 64 + ql + 1 + FM_LS_BIAS) << 1) | hb;
    }
    if (tid < 64) {
        int64_t q = -1;
        bool found = t0 == 0;
        // whether the line after the newline at q is a header: the byte after q, taken from the
        // window that holds q (a shuffle), from the window after it (its first byte, kept from the
        // previous step) or, for a newline at t0 - 1, from the tile's own first byte
        uint32_t hb = tile_first;          // t0 == 0, or q == t0 - 1
        uint32_t next_first = tile_first;  // '>' flag of the byte after the current window
        for (int step = 0; step < FM_SCAN_BYTES / 1024 && !found; ++step) {
            if (t0 < (uint64_t)(step + 1) * 1024) break;
            const uint64_t a0 = t0 - (uint64_t)(step + 1) * 1024, a = a0 + 16 * (uint64_t)tid;
            uint32_t w4[4];
            if (step == 0) {
#pragma unroll
                for (int i = 0; i < 4; ++i) w4[i] = rb0[i];
            } else {
                load_rb(a, w4);
            }
            uint32_t m16 = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) m16 |= zero_bytes4(w4[i] ^ 0x0a0a0a0au) << (4 * i);
            const int64_t mine = m16 ? (int64_t)(a + 31 - __builtin_clz(m16)) : -1;
            q = __shfl(wave_incl_max<int64_t>(mine), 63, 64);
            found = q >= 0;
            if (found) {  // uniform
                const uint64_t rel = (uint64_t)(q + 1) - a0;  // 1 .. 1024
                if (rel < 1024) {
                    const uint32_t bi = (uint32_t)rel & 15u, wi = bi >> 2;
                    const uint32_t w = wi == 0 ? w4[0] : (wi == 1 ? w4[1] : (wi == 2 ? w4[2] : w4[3]));
                    const uint32_t byte = (uint32_t)__shfl((int)((w >> (8 * (bi & 3u))) & 0xffu), (int)(rel >> 4), 64);
                    hb = byte == '>' ? 1u : 0u;
                } else {
                    hb = next_first;
                }
            }
            next_first = (uint32_t)__shfl((int)(w4[0] & 0xffu), 0, 64) == '>' ? 1u : 0u;
        }
        if (tid == 0) {
            if (!found) atomicOr(&counters[2], (unsigned long long)FM_FB_LINE);
            if (fa_first != '>') atomicOr(&counters[2], (unsigned long long)FM_FB_JUNK);
            // line start after that newline (<= t0: an earlier byte or the tile's first); later
            // threads without a newline of their own continue this line
            const uint64_t ls = t0 == 0 ? 0 : (uint64_t)(q + 1);
            s_bcast[0] = found ? (((uint32_t)(ls + FM_LS_BIAS - t0) << 1) | hb) : ((uint32_t)FM_LS_BIAS << 1);
        }
    }
    uint32_t tile_last;
    // (no trailing barrier: s_tmp32 is not written again)
    const uint32_t excl = block_excl_max<uint32_t, false, NTH>(val, 0u, s_tmp32, &tile_last);
    const uint32_t prev = max(excl, (uint32_t)s_bcast[0]);
    const uint64_t ls = t0 + (prev >> 1) - FM_LS_BIAS;
    const bool ls0 = nb > 0 && ls == p0;
    const uint64_t cin = (nb > 0 && !ls0 && (prev & 1u)) ? 1ull : 0ull;
    const uint64_t H = ((nl << 1) | (ls0 ? 1ull : 0ull)) & gt;  // header starts ('>' at a line start)
    const uint64_t X = ~nl;
    const uint64_t hdr = X ^ (X + H + cin);
    uint64_t notjunk = ~0ull;
    if (tile == 0) {  // lines before the first header of the input are not sequence
        int64_t neg_first;
        (void)block_excl_max<int64_t, true, NTH>(H ? -(int64_t)(p0 + __builtin_ctzll(H)) : -INT64_MAX, -INT64_MAX,
                                                 s_tmp64, &neg_first);
        const int64_t fh = -neg_first;
        if (fh >= (int64_t)(p0 + 64))
            notjunk = 0ull;
        else if (fh > (int64_t)p0)
            notjunk = ~0ull << (fh - (int64_t)p0);
    }
    const uint64_t kept = ((~nl & ~hdr) | H) & notjunk & inr;
    const uint64_t vbits = kept & ok;
    FM_STAMP(1);  // line state (read-back, block max-scan)
    if (probe == 1) {  // timing probe (FASTKMER_FUSED_PROBE): stop after the byte classes and line state
        if ((kept ^ vbits ^ clo ^ chi) == 0x0123456789abcdefull) counters[6] = kept;
        return;
    }

    // ---- 2. compaction into tile-local LDS streams (MSB-first).  Each 32-byte half is compacted
    // run by run on 64-bit code words (LSB-first), then the halves are joined.
    const uint32_t my_off = block_excl_sum<uint32_t, false, NTH>((uint32_t)__popcll(kept), s_sum, &P_all);
    if (tid == NTH - FM_HALO_T) s_pown = my_off;
    {
        uint64_t alo = 0, ahi = 0;
        uint32_t vlo = 0, vhi = 0;
        int nlo = 0, nhi = 0;
        fm_compact32((uint32_t)kept, clo, (uint32_t)vbits, alo, vlo, nlo);
        fm_compact32((uint32_t)(kept >> 32), chi, (uint32_t)(vbits >> 32), ahi, vhi, nhi);
        const int na = nlo + nhi;
        if (na) {
            // 128-bit stream acc = alo | ahi << 2 nlo, 64-bit valid stream vacc = vlo | vhi << nlo
            const u128 acc = (u128)alo | ((u128)ahi << (2 * nlo));
            const uint64_t vacc = (uint64_t)vlo | ((uint64_t)vhi << nlo);
            const int sh = 2 * (my_off & 15);
            const u128 lo = acc << sh;
            const uint32_t hi = sh ? (uint32_t)(acc >> (128 - sh)) : 0u;
            const int nw = (sh + 2 * na + 31) >> 5;
            uint32_t *dst = &s_code[my_off >> 4];
            // each partial word is turned MSB-first before it is ORed in (a bit permutation commutes
            // with OR), so there is no in-place reversal pass and no barrier for it
            auto msb_codes = [](uint32_t x) {
                x = __builtin_bitreverse32(x);
                return ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
            };
            auto msb_valid = [](uint32_t x) { return __builtin_bitreverse32(x); };
#pragma unroll
            for (int j = 0; j < 5; ++j)
                if (j < nw) atomicOr(&dst[j], msb_codes(j < 4 ? (uint32_t)(lo >> (32 * j)) : hi));
            const int shv = my_off & 31;
            const uint64_t vl = vacc << shv;
            const uint32_t vh = shv ? (uint32_t)(vacc >> (64 - shv)) : 0u;
            const int nwv = (shv + na + 31) >> 5;
            uint32_t *dv = &s_valid[my_off >> 5];
            atomicOr(&dv[0], msb_valid((uint32_t)vl));
            if (nwv > 1) atomicOr(&dv[1], msb_valid((uint32_t)(vl >> 32)));
            if (nwv > 2) atomicOr(&dv[2], msb_valid(vh));
        }
    }
    __syncthreads();
    FM_STAMP(2);  // compaction into LDS (MSB-first)
    if (probe == 2) {  // stop after the compaction
        if (s_code[tid] == 0x01234567u && s_valid[tid & 63] == 0x89abcdefu) counters[6] = tid;
        return;
    }
    P_own = s_pown;
    {  // the tile's code stream, as far as its records read it (a record starting at p < P_own reads
       // words p / 16 .. p / 16 + 5, see src_build); MODE 1: whole, with the valid stream and the
       // position counts, for the passes of MODE 2
        uint32_t *tc = codes + tile * (uint64_t)FM_CSLOT;
        const uint32_t nw = MODE == 1 ? (uint32_t)Gm::CODE_WORDS : min<uint32_t>((uint32_t)Gm::CODE_WORDS, (P_own >> 4) + 8u);
        for (uint32_t i = tid; i < nw; i += NTH) tc[i] = s_code[i];
        if constexpr (MODE == 1) {
            for (uint32_t i = tid; i < (uint32_t)Gm::VALID_WORDS; i += NTH) vs[4 + i] = s_valid[i];
            if (tid == 0) vs[0] = P_own, vs[1] = P_all;
        }
    }
    // an owned window is undecided when it starts after the last invalid position of the tile's
    // stream ('>' of a header, N, lowercase, ...) and runs past the parsed bytes (the halo held
    // too few positions), unless the input ends there; the block scan for the last invalid
    // position runs only for tiles whose halo is that short (uniform condition)
    if ((more || t0 + Gm::SPAN < n) && P_own > 0 && P_own - 1 + (uint32_t)k > P_all) {
        const uint64_t inv = kept & ~ok;
        int mine = -1;
        if (inv) mine = (int)my_off + __popcll(kept & low_mask(64 - __clzll(inv))) - 1;
        int last_inv;
        (void)block_excl_max<int, true, NTH>(mine, -1, s_tmpi, &last_inv);
        if (tid == 0 && last_inv < (int)P_own - 1) atomicOr(&counters[2], (unsigned long long)FM_FB_HALO);
    }
    if constexpr (MODE == 1) return;  // the passes: MODE 2
    }  // parse (MODE 0 / 1)

    // ---- 3. signature passes, one wave per pass of PL * 16 positions, no workgroup barrier
    // Lane l of a pass owns the windows starting at base + 16 l .. +15 (l < PL); the last 64 - PL
    // lanes only supply norms: the window minima come from each lane's prefix / suffix minima and
    // its successors' prefix minima (DPP lane shifts).  Runs of equal signature are cut every 16
    // k-mers and at pass ends.  A pass claims its records' slots in the tile with one LDS atomic,
    // queues the record starts (positions) per lane, then the wave completes and stores the
    // records in converged steps (signature from the wave's scratch copy of the window minima).
    constexpr int JMAX = (15 + w - 1) >> 4;  // farthest successor lane a window reaches
    constexpr int PL = 64 - JMAX;            // lanes owning windows
    constexpr int PSTRIDE = PL * 16;
    constexpr int NW = NTH / 64;
    const int lane = tid & 63, wid = tid >> 6;
    const bool pow2_bins = (fm.d & (fm.d - 1u)) == 0u;
    uint32_t *wscr = s_wscr + wid * 1024;
    uint32_t *wstop = s_wstop + wid * 64;
    uint32_t *wq = s_wq + wid * FM_QCAP;
    uint32_t *thdr = hdrs + tile * (uint64_t)FM_TCAP;  // this tile's record slots: header words
    uint16_t *tpos = pos + tile * (uint64_t)FM_TCAP;   // and first positions
    uint32_t nk = 0;    // per lane: valid windows
    bool wovf = false;  // uniform
    const uint32_t npass = (P_own + PSTRIDE - 1) / PSTRIDE;
    FM_STAMP(3);  // code-stream store, halo check
    for (uint32_t pass = wid; pass < npass; pass += NW) {
        const uint32_t base = pass * PSTRIDE;
        const uint32_t i0 = base + (uint32_t)lane * SIG_PPT;
        uint32_t pre[16], suf[16];
        // complemented norms: window maxima of ~norm = ~(window minima of norm), every DPP
        // hop a bound_ctrl move (0 = the identity of max: no identity register, hops fused into v_max)
        uint32_t wmin[16];  // ~ window minimum
        {
            uint32_t own[16];
            fm_norm_block<MC, true>(s_code, (int)(i0 >> 4), own);
            pre[0] = own[0];
#pragma unroll
            for (int s = 1; s < 16; ++s) pre[s] = max(pre[s - 1], own[s]);
            suf[15] = own[15];
#pragma unroll
            for (int s = 14; s >= 0; --s) suf[s] = max(own[s], suf[s + 1]);
            auto shl1 = [](uint32_t x) {  // lane + 1's value, 0 past the last lane (wave_shl:1, bound_ctrl)
                return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x130, 0xf, 0xf, true);
            };
            uint32_t P[JMAX][16];
#pragma unroll
            for (int x = 0; x < 16; ++x) P[0][x] = shl1(pre[x]);
#pragma unroll
            for (int j = 1; j < JMAX; ++j)
#pragma unroll
                for (int x = 0; x < 16; ++x) P[j][x] = shl1(P[j - 1][x]);
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                const int e = s + w - 1;  // window end relative to i0
                const int J = e >> 4, r = e & 15;
                uint32_t v = max(suf[s], P[J - 1][r]);
#pragma unroll
                for (int j = 1; j < J; ++j) v = max(v, P[j - 1][15]);
                wmin[s] = v;
            }
        }
        // valid windows of the 16 starts: bit s <-> window at i0 + s (owned positions only)
        uint32_t vmask;
        {
            const uint32_t q = i0 >> 5;
            if constexpr (KC + 15 <= 64) {
                uint64_t V = ((uint64_t)s_valid[q] << 32) | s_valid[q + 1];
                if (i0 & 16) V = (V << 16) | (s_valid[q + 2] >> 16);
                uint64_t R = V;
                int a = 1;
                while (2 * a <= k) {
                    R &= R << a;
                    a <<= 1;
                }
                const uint64_t okw = R & (R << (k - a));
                vmask = __builtin_bitreverse32((uint32_t)(okw >> 48)) >> 16;
            } else {
                u128 V = ((u128)s_valid[q] << 96) | ((u128)s_valid[q + 1] << 64) | ((u128)s_valid[q + 2] << 32) |
                         (u128)s_valid[q + 3];
                if (i0 & 16) V = (V << 16) | (u128)(s_valid[q + 4] >> 16);
                u128 R = V;
                int a = 1;
                while (2 * a <= k) {
                    R &= R << a;
                    a <<= 1;
                }
                const u128 okw = R & (R << (k - a));
                vmask = __builtin_bitreverse32((uint32_t)(okw >> 112)) >> 16;
            }
            const int lim = lane < PL ? (int)P_own - (int)i0 : 0;
            vmask &= lim >= 16 ? 0xffffu : (lim <= 0 ? 0u : ((1u << lim) - 1u));
        }
        nk += (uint32_t)__popc(vmask);
        // runs of equal signature, cut every 16 k-mers from the run start (as k_superkmers)
        const uint32_t psig = dppz<0x138>(wmin[15]), pvmask = dppz<0x138>(vmask);  // wave_shr:1
        // bit s = (wmin[s] != wmin[s - 1]): one compare and one add-with-carry per bit (the compiler's
        // select + OR costs 2.5)
        uint32_t neq = 0u;
#pragma unroll
        for (int s = 15; s >= 1; --s) neq = fm_push_ne(neq, wmin[s], wmin[s - 1]);
        neq = fm_push_ne(neq, wmin[0], psig);
        const uint32_t pvm = (vmask << 1) | ((pvmask >> 15) & 1u);
        const uint32_t rs = vmask & (~pvm | neq);
        const int mine_rs = rs ? (int)i0 + 31 - __builtin_clz(rs) : -1;
        const int prev_rs = (int)dppz<0x138>(wave_incl_max<uint32_t>((uint32_t)(mine_rs + 1))) - 1;  // exclusive
        const int pc = prev_rs & 15;
        const bool cut = ((rs & ((2u << pc) - 1u)) == 0u) && ((vmask >> pc) & 1u);
        const uint32_t starts = rs | (cut ? 1u << pc : 0u);
        const uint32_t stops = (~vmask | starts) & 0xffffu;
        // wave_shl:1 (the last lane owns no windows: its successor's stops are never read)
        const uint32_t nstops = dppz<0x130>(stops);
        const uint32_t cnt = (uint32_t)__popc(starts);
        const uint32_t inc = wave_incl_sum_z(cnt);
        const uint32_t T = (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
        FM_STAMP(4);  // signature pass: norms, window minima, run starts, scans
        if (probe == 3) {  // timing probe: the signature passes without the records
            if (T == 0x7fffffffu) counters[6] = inc;
            continue;
        }
        if (T == 0 || wovf) continue;
        uint32_t slot = 0;
        if (lane == 0) slot = atomicAdd(&s_tcnt, T);
        slot = (uint32_t)__builtin_amdgcn_readfirstlane((int)slot);
        if (slot + T > (uint32_t)FM_TCAP) {
            wovf = true;
            continue;
        }
        // the wave's window minima and stop masks, for the converged completion below
#pragma unroll
        for (int g = 0; g < 4; ++g)
            *reinterpret_cast<uint4 *>(wscr + fm_scr((uint32_t)lane, 4u * g)) =
                make_uint4(wmin[4 * g], wmin[4 * g + 1], wmin[4 * g + 2], wmin[4 * g + 3]);
        wstop[lane] = stops | (nstops << 16);
        for (uint32_t c0 = 0; c0 < T; c0 += FM_QCAP) {
            if (probe == 4) {  // timing probe: queue the starts, build no records
                if (c0 == 0x7fffffffu) counters[6] = T;
                break;
            }
            // record starts (positions) with pass rank in [c0, c0 + QCAP) into the wave's queue
            uint32_t st = starts, r = inc - cnt - c0;
            while (st) {
                const int s = __builtin_ctz(st);
                st &= st - 1;
                if (r < (uint32_t)FM_QCAP) wq[r] = i0 + (uint32_t)s;
                ++r;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const uint32_t nq = min(T - c0, (uint32_t)FM_QCAP);
            for (uint32_t j = (uint32_t)lane; j < nq; j += 64) {
                const uint32_t a = wq[j];
                const uint32_t rel = a - base, ol = rel >> 4, sp = rel & 15u;
                const uint32_t sig = ~wscr[fm_scr(ol, sp)];  // the scratch holds complements
                const uint32_t after = wstop[ol] & ~((2u << sp) - 1u);  // a stop lies within 16 positions
                const int nn = __builtin_ctz(after) - (int)sp;
                const uint32_t bin = pow2_bins ? (hash32(sig) & (fm.d - 1u)) : bin_of_signature(sig, fm);
                // the compact record: header (bin, n - 1, fine hash) and the first position
                const uint64_t idx = slot + c0 + j;
                thdr[idx] = bin | ((uint32_t)(nn - 1) << REC_BIN_BITS) | (fine_of_signature(sig) << REC_FINE_SHIFT);
                tpos[idx] = (uint16_t)a;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
        FM_STAMP(5);  // record slots, queue, completion, stores
    }
    FM_STAMP(6);  // (passes skipped)
    {
        const uint32_t nkw = (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_sum<uint32_t>(nk), 63);
        if (lane == 0) {
            s_wnk[wid] = nkw;
            if (wovf) s_wovf = 1u;
        }
    }
    __syncthreads();
    FM_STAMP(7);  // the workgroup's last barrier (waves done with their passes wait here)
    if (tid == 0) {
        uint32_t nkt = 0;
#pragma unroll
        for (int v = 0; v < NW; ++v) nkt += s_wnk[v];
        const uint32_t nrec = s_wovf ? 0u : s_tcnt;
        tcnt[tile] = nrec;
        if (s_wovf) atomicOr(&counters[2], (unsigned long long)FM_FB_DESC);
        if (probe == 0) {  // summed by k_tile_totals (same-address atomics of every tile serialize)
            tstat[2 * tile] = nkt;
            tstat[2 * tile + 1] = P_own;
        }
    }
    }
    FM_FLUSH();
}

// (k, m) pairs with a fused instantiation (the BASELINE configurations)
bool map_fused_supported(int k, int m, uint32_t nbins) {
    if (nbins > REC_BIN_MASK + 1u) return false;
    return (k == 28 && m == 10) || (k == 55 && m == 12);
}

#ifdef FK_PROBES
hipError_t map_fused_cycles(unsigned long long *out16, bool reset) {
    static unsigned long long rows[FM_CYC_ROWS * 16];
    hipError_t e = hipMemcpyFromSymbol(rows, HIP_SYMBOL(g_fm_cycles), sizeof rows, 0, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return e;
    for (int i = 0; i < 16; ++i) {
        out16[i] = 0;
        for (int r = 0; r < FM_CYC_ROWS; ++r) out16[i] += rows[r * 16 + i];
    }
    if (reset) {
        for (auto &v : rows) v = 0;
        e = hipMemcpyToSymbol(HIP_SYMBOL(g_fm_cycles), rows, sizeof rows, 0, hipMemcpyHostToDevice);
    }
    return e;
}
#else
hipError_t map_fused_cycles(unsigned long long *, bool) { return hipErrorNotSupported; }
#endif

uint32_t map_fused_tcap() { return (uint32_t)FM_TCAP; }
uint32_t map_fused_cslot() { return (uint32_t)FM_CSLOT; }
uint32_t map_fused_vslot() { return (uint32_t)FM_VSLOT; }

// counters[0] = sum of tcnt, [1] / [3] = sums of the tiles' k-mers / positions (one workgroup)
__global__ __launch_bounds__(1024) void k_tile_totals(const uint32_t *__restrict__ tcnt,
                                                      const uint32_t *__restrict__ tstat, uint64_t ntiles,
                                                      unsigned long long *counters) {
    __shared__ unsigned long long s_part[3][1024 / 64];
    unsigned long long r = 0, km = 0, ps = 0;
    for (uint64_t t = threadIdx.x; t < ntiles; t += 1024) {
        r += tcnt[t];
        km += tstat[2 * t];
        ps += tstat[2 * t + 1];
    }
    r = wave_incl_sum<unsigned long long>(r);
    km = wave_incl_sum<unsigned long long>(km);
    ps = wave_incl_sum<unsigned long long>(ps);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 63) s_part[0][wid] = r, s_part[1][wid] = km, s_part[2][wid] = ps;
    __syncthreads();
    if (threadIdx.x < 3) {
        unsigned long long acc = 0;
        for (int w = 0; w < 1024 / 64; ++w) acc += s_part[threadIdx.x][w];
        counters[threadIdx.x == 0 ? 0 : (threadIdx.x == 1 ? 1 : 3)] = acc;
    }
}

hipError_t launch_tile_totals(const uint32_t *tcnt, const uint32_t *tstat, uint64_t ntiles,
                              unsigned long long *counters, hipStream_t s) {
    k_tile_totals<<<1, 1024, 0, s>>>(tcnt, tstat, ntiles, counters);
    return hipGetLastError();
}

// vslots (map_fused_vslot() words per tile of the launch; a -DFK_PROBES library only): the map in two
// kernels -- the parse (MODE 1: code and valid streams to HBM) then the signature passes (MODE 2: the
// streams back into LDS), a measurement of the two phases apart; null: one fused kernel (MODE 0)
hipError_t launch_map_fused(int nth, int k, int m, const uint8_t *fa, uint64_t n, int more, uint64_t tile_begin,
                            uint64_t ntiles, FastMod fm, uint32_t *hdrs, uint16_t *pos, uint32_t *codes,
                            uint32_t *tcnt, uint32_t *tstat, unsigned long long *counters, hipStream_t s, int probe,
                            uint32_t *vslots) {
    if (ntiles == 0) return hipSuccess;
    if (!map_fused_supported(k, m, fm.d) || nth != FM_NT) return hipErrorInvalidValue;
    if (vslots && probe) return hipErrorInvalidValue;
    const unsigned g = (unsigned)ntiles;
#define FK_FUSED(NTH_, K_, M_, MODE_)                                                                        \
    k_map_fused<NTH_, K_, M_, MODE_><<<g, NTH_, 0, s>>>(fa, n, more, tile_begin, fm, hdrs, pos, codes, tcnt, \
                                                        tstat, vslots, counters, probe)
    if (vslots) {
#ifdef FK_PROBES
        if (k == 28) {
            FK_FUSED(FM_NT, 28, 10, 1);
            FK_FUSED(FM_NT, 28, 10, 2);
        } else {
            FK_FUSED(FM_NT, 55, 12, 1);
            FK_FUSED(FM_NT, 55, 12, 2);
        }
#else
        return hipErrorNotSupported;
#endif
    } else if (k == 28) {
        FK_FUSED(FM_NT, 28, 10, 0);
    } else {
        FK_FUSED(FM_NT, 55, 12, 0);
    }
#undef FK_FUSED
    return hipGetLastError();
}
