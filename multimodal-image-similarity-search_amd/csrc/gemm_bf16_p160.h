// gemm_bf16_p160.h — 160 x 256 x 64 bf16 GEMM tile on a staggered two-barrier loop (the discipline of gemm_bf16_p256.h), for
// the NARROW GEMMs of a ViT-B/32 layer on the bf16 residual stream (MMISS_EPI_BIAS_RESID_BF16: out = bf16(f32(out) + A W^T +
// bias) in place, + the row statistics of the new rows): out-projection 12800 x 768 x 768 and FC2 12800 x 768 x 3072.
//
// Why this tile: 12 800 rows x 768 columns are 150 tiles of 256 x 256 — 0.59 of the chip — and 300 of 128 x 256; as 160 x 256
// they are 80 x 3 = 240 workgroups = ONE round on 256 CUs. The 160 x 128 tile of gemm_bf16.h (the same 240-wide grid, two
// workgroups per CU) runs the older loop — one barrier per K-tile behind an s_waitcnt vmcnt(0) — at 0.86-0.96 PF on FC2;
// stream-K over 256 x 256 tiles lost the operand sharing between neighbouring workgroups and was slower
// (profiles/gemm_p256_r03.txt, section 9).
//   * 8 waves as 2 (m) x 4 (n): a wave owns 80 rows x 64 columns = 5 x 4 accumulator blocks of 16 x 16.
//   * TWO phases per K-tile, one per K STEP of 32 columns — [5 A + 4 W fragment reads, staging] B [20 MFMAs] B, twice — with the
//     two wave halves one barrier apart (one half's read part beside the other's MFMAs). Measured on FC2, us per K-tile net of
//     the launch's ~12 us of fill, prefetch and epilogue (round 3, ablation builds since removed; the 80 MFMAs alone take 0.58, the 52 KB
//     of LDS-DMA alone 0.62-0.67, the 36 fragment reads alone 0.29-0.35): the four quadrant phases of the 256 x 256 tile
//     (12 / 12 / 8 / 8 MFMAs; 80 rows do not halve evenly) 1.3; two staggered phases split by n half (14 + 4 reads) 1.06; these
//     two (9 + 9 reads) 0.96; an unstaggered form with two fragment sets in registers (a wave reads the next phase's fragments,
//     then issues this phase's MFMAs) 1.03. Whatever the order, MFMAs + fragment reads take their SUM (0.88 without staging):
//     on this machine a 1 KB fragment landing in the register file costs the matrix pipe what an MFMA's 1 KB of results
//     costs it, and an 80 x 64 wave tile needs 9 fragments per 20 MFMAs. FC2 ends at 0.97-0.99 PF instead of 0.90.
//   * THREE staging buffers of 52 KB (A 160 rows, W n0 / n1 128 rows each), K-tile t+2 staged while t is computed: a K-tile is
//     ~0.9 us here, two of them in flight (104 KB per CU) keep the prefetch distance of the 256 x 256 loop in time.
//   * 20 A pieces of 8 rows for 8 waves: every wave issues THREE LDS-DMA operations for the A slot (waves 4-7: two pieces and a
//     4-byte-per-lane filler into a dump area) and two per W slot — 7 per K-tile on every wave, so one counted wait serves all.
//   * one tile per workgroup: the bf16 rows it adds to (its own output rows, 80 KB) are fetched UNDER the K loop, by the two
//     stagings that have no K-tile left to fetch (issued during K-tiles nt - 2 and nt - 1; they used to wrap round and re-read
//     K-tiles 0 and 1 for nobody) — same instructions, other descriptor and offsets — into the LDS slots those fill; a wave
//     reads back only pieces it issued itself, so its own waits cover them (the first staging: the K loop's last vmcnt(7);
//     the second: one vmcnt(0) in front of the wave's first output store), and the barrier behind the loop, which was always
//     there, only frees the last fragment buffer. The epilogue reads them from LDS in the accumulator layout. Nothing
//     of them is older than K-tile 0's pieces: they used to be 24 register loads in front of the prologue, which the
//     prologue's first counted wait had to sit out (vector-memory operations retire in order) and which held 40 VGPRs
//     through the loop. Only the bias (1 KB) is still requested ahead. The epilogue's transpose patches lie over the one
//     staging buffer those two stagings do not fill, (nt - 1) % 3 (the patch-embedding GEMM: buffer 0).
//   * the residual epilogue is fully exposed (one tile per workgroup, all 240 enter it together), so it is written for its
//     instruction count (profiles/gemm_p160_epilogue.txt: 1102 -> 759 instructions behind the last MFMA, 52 -> 16 waits). The
//     row statistics were 60 % of it: their eight-lane sums are DPP adds (no ds_bpermute, no LDS wait), two rows' four chains
//     interleaved; statistics and rows leave through buffer stores whose per-lane offsets are fixed per tile (block steps
//     are scalar), the statistics predicated by the descriptor's range check in place of ten exec-mask branches. Two
//     patches per wave alternate, so block j + 1 is packed and written while block j's read-back is on its way, and blocks
//     0..2 start on the first late staging while the second is still in flight (what each block reads: at the epilogue).
//     The output rows are stored sc1 (written through): nothing is left dirty in the L2s for the kernel's end.
//   * the patch-embedding GEMM straight from the f32 pixels (MMISS_EPI_PATCH_PIX_F32): its A operand is the [B,3,S,S] image,
//     not an im2col copy. Tile row r is patch (img, py, px), K index k is (c, ky, kx), so a 64-wide K-tile of a row is 64 / P
//     pixel-row segments of P floats. The A slot's 8-row pieces keep their owners and their swizzle; a lane fetches 16 bytes of the K-tile's
//     first and of its second 32 floats (eight lanes: 128 contiguous bytes), converts with im2col_kernel's pack_bf16x2 and writes
//     the two half chunks where the LDS-DMA would have put them. hipcc drains vmcnt(0) at the first use of an ordinary load's result while LDS-DMA is in
//     flight, so these loads are inline asm it does not count, their destinations named by the counted wait in front of their
//     first use. Two register sets: K-tile t + 2's pixels are requested in phase 0 of K-tile t and written to LDS in phase 1
//     of K-tile t + 1 (a K-tile and a half of latency cover), read from K-tile t + 2 on. A wave has 6 loads + 4 LDS-DMA in
//     flight per K-tile: the waits are vmcnt(10). Same K order in every accumulator and the same epilogue as the bf16 form.
// Fragment layout and swizzle: gemm_bf16_p256.h.
#pragma once
#include "gemm_bf16_256.h"

// internal: MMISS_EPI_PATCH_F32 with the A operand read from the f32 pixels (ep.pix_S, ep.pix_P, ep.pix_bytes); gemm160p_kernel only
#define MMISS_EPI_PATCH_PIX_F32 10

#define G160_A_BYTES 20480                  // 160 rows x 128 B
#define G160_W_BYTES 16384                  // 128 rows x 128 B
#define G160_BUF (G160_A_BYTES + 2 * G160_W_BYTES)   // one K-tile: A | W n0 | W n1
#define G160_DUMP (3 * G160_BUF)            // 8 waves x 256 B: where the 4-byte filler pieces land
#define G160_LDS (G160_DUMP + 2048)         // 161 792 B of the CU's 163 840

// Four values per lane, each added up over the eight lanes that share lane >> 3, by DPP adds instead of LDS permutes: xor 1 and
// xor 2 within the quad (partner's + own: what v += __shfl_xor(v, 1 / 2) gives, x + y and y + x being the same bits), after
// which a quad's four lanes hold one value, so the xor 4 step may take any lane of the other quad: the half-row mirror, lane l
// of the eight <- lane 7 - l. Written as instructions because the compiler, which pairs the sums into packed adds, keeps a
// v_mov_b32_dpp and two copies in front of every one of them. A DPP source must have been written at least two instructions
// earlier: the leading s_nop covers whatever wrote the inputs, the four independent chains cover one another. The compiler
// sees none of this inside the asm. What it ASSUMES of the caller: no VALU instruction writes EXEC (v_cmpx, v_readlane-style
// masks) within five instructions in front of the call — a DPP instruction needs five wait states behind such a write. The
// epilogue calls it from straight-line code under the full exec mask; anyone who puts it behind an exec-masked branch
// makes the leading wait s_nop 4.
__device__ __forceinline__ void g160_row_sum8(float& a, float& b, float& c, float& d) {
#define G160_DPP4(ctrl)                                              \
    "v_add_f32_dpp %0, %0, %0 " ctrl " row_mask:0xf bank_mask:0xf\n\t" \
    "v_add_f32_dpp %1, %1, %1 " ctrl " row_mask:0xf bank_mask:0xf\n\t" \
    "v_add_f32_dpp %2, %2, %2 " ctrl " row_mask:0xf bank_mask:0xf\n\t" \
    "v_add_f32_dpp %3, %3, %3 " ctrl " row_mask:0xf bank_mask:0xf\n\t"
    asm("s_nop 1\n\t" G160_DPP4("quad_perm:[1,0,3,2]") G160_DPP4("quad_perm:[2,3,0,1]") G160_DPP4("row_half_mirror")
        : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
#undef G160_DPP4
}

// (sum, sum of squares) of a lane's eight stored bf16 values, in gemm_epilogue's order. Every product and every sum is
// rounded on its own, as the compiler has always built this loop: a contraction into FMAs, which it is otherwise free to
// choose with the code around the loop, would change the statistics' bits.
__device__ __forceinline__ void g160_row_part(const u32x4& pk, float& rs, float& rq) {
#pragma clang fp contract(off)
    rs = 0.f;
    rq = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float a = __uint_as_float(pk[e] << 16), b = __uint_as_float(pk[e] & 0xFFFF0000u);
        rs += a + b;
        rq += a * a + b * b;
    }
}

// EPI: MMISS_EPI_BIAS_RESID_BF16 (the residual GEMMs) or MMISS_EPI_PATCH_F32 (the patch-embedding GEMM: f32 rows scattered to
// item * tokens + 1 + patch with the position row added, gemm_bf16.h gemm_epilogue's contract; no bias, no residual).
// KT: the K-tile count as a compile-time tag (0 = read K at run time). It exists so that the shapes of one encode are
// DISTINCT SYMBOLS in rocprofv3's kernel trace and PMC passes — out-projection (K = 768: <9,12>) and FC2 (K = 3072: <9,48>)
// were one symbol with a 24-75 us "class average" in round 3 — and gives the K loop a constant trip count.
template <int EPI, int KT = 0>
__global__ __launch_bounds__(512, 2) void gemm160p_kernel(const __bf16* __restrict__ A, const __bf16* __restrict__ W, int M,
                                                          int N, int K, GemmEpi ep) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    typedef bf16x8 frag;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;
    const int fr = lane & 15, fg = lane >> 4;
    const int nbm = M / 160, nbn = N >> 8;
    const int nt = KT > 0 ? KT : K / GEMM_BK;  // even (K % 128 == 0)
    const int wg = xcd_remap(blockIdx.x, nbm * nbn);
    int bm, bn;
    tile_order(wg, nbm, nbn, 0, bm, bn);   // n fastest: the column tiles of a row block run side by side on one XCD
    const __bf16* Ab = A + (size_t)bm * 160 * K;
    const __bf16* Wb = W + (size_t)bn * 256 * K;

    // ---- LDS-DMA sources, buffer form: one per-lane offset (row r_in of an 8-row piece, swizzled 16-byte chunk), everything
    // else scalar. A slot row r = tile row r; piece q = rows 8q .. 8q+7 at q * 1024. W slot row r = weight row
    // (r >> 5) * 64 + nq * 32 + (r & 31) (the 32 rows of n half nq of each of the four wave columns).
    //
    // Everything a staging operation READS is a run-time value — descriptor, per-lane offset, the seven scalar offsets — so
    // that the residual GEMMs can point the two stagings past the last K-tile at their own old output rows (G160_NEXT_KTILE)
    // through the SAME instructions: there is one copy of the K-tile body. Where it WRITES never changes.
    constexpr bool RESID = (EPI == MMISS_EPI_BIAS_RESID_BF16);
    constexpr bool PIX = (EPI == MMISS_EPI_PATCH_PIX_F32);
    constexpr bool PATCH = (EPI == MMISS_EPI_PATCH_F32) || PIX;
    static_assert(RESID || PATCH, "gemm160p_kernel: epilogue");
    const int r_in = lane >> 3, p = lane & 7;
    int lane_vo = (r_in * K + ((p ^ r_in) * 8)) * 2;
    __amdgpu_buffer_rsrc_t srdA = __builtin_amdgcn_make_buffer_rsrc(const_cast<__bf16*>(Ab), 0, 0x7fffffff, 0x00020000);
    __amdgpu_buffer_rsrc_t srdW = __builtin_amdgcn_make_buffer_rsrc(const_cast<__bf16*>(Wb), 0, 0x7fffffff, 0x00020000);
    const int row8 = 8 * K * 2;                 // bytes between two consecutive 8-row pieces
    const int a_so = wave * row8;               // A pieces w, w + 8 and (waves 0-3) w + 16
    const int a_dst = wave * 1024;
    const int w_so = ((wave >> 1) * 64 + (wave & 1) * 16) * K * 2;   // W slot rows 16w, 16w + 8; the n1 slot is 32 weight rows on
    const int w_dst = wave * 2048;
    int xa0 = a_so, xa1 = a_so + 8 * row8, xa2 = a_so + 16 * row8, xaf = a_so;           // A pieces; the filler's source
    int xw0 = w_so, xw1 = w_so + row8, xw2 = w_so + 4 * row8, xw3 = w_so + 5 * row8;     // W n0 (two pieces), W n1 (two)
    int kstep = GEMM_BK * 2;                    // what ko2 advances by per K-tile
// (the patch-embedding GEMM never re-points them: it keeps the expressions, and with them its instructions, as they were)
#define G160_X(var, expr) (RESID ? (var) : (expr))
    char* const dump = smem + G160_DUMP + wave * 256;
#define G160_BLDS(srd, so, dst) \
    __builtin_amdgcn_raw_ptr_buffer_load_lds(srd, (__attribute__((address_space(3))) void*)(dst), 16, lane_vo, so, 0, 0)
#define G160_FILL(srd, so) \
    __builtin_amdgcn_raw_ptr_buffer_load_lds(srd, (__attribute__((address_space(3))) void*)(dump), 4, lane_vo, so, 0, 0)
// the A slot of buffer b2 <- K-tile at byte offset ko: THREE operations per wave
#define G160_STAGE_A(b2, ko)                                                                                 \
    {                                                                                                       \
        char* sl_ = smem + (b2) * G160_BUF + a_dst;                                                         \
        G160_BLDS(srdA, G160_X(xa0, a_so) + (ko), sl_);                                                     \
        G160_BLDS(srdA, G160_X(xa1, a_so + 8 * row8) + (ko), sl_ + 8 * 1024);                               \
        if (wave < 4) { G160_BLDS(srdA, G160_X(xa2, a_so + 16 * row8) + (ko), sl_ + 16 * 1024); }           \
        else { G160_FILL(srdA, G160_X(xaf, a_so) + (ko)); }                                                 \
    }
// the W slot of n half nq: TWO operations per wave
#define G160_STAGE_W(b2, nq, ko)                                                                             \
    {                                                                                                       \
        char* sl_ = smem + (b2) * G160_BUF + G160_A_BYTES + (nq) * G160_W_BYTES + w_dst;                    \
        const int so_ = G160_X((nq) ? xw2 : xw0, w_so + (nq) * 4 * row8) + (ko);                            \
        G160_BLDS(srdW, so_, sl_);                                                                          \
        G160_BLDS(srdW, G160_X(((nq) ? xw3 : xw1) + (ko), so_ + row8), sl_ + 1024);                         \
    }

    // ---- the old rows of the residual GEMMs (the bf16 rows this workgroup adds to: its own output rows, nobody else touches
    // them) ride in the two stagings that have no K-tile left to fetch — the ones issued during K-tiles nt - 2 and nt - 1, into
    // buffers nt % 3 and (nt + 1) % 3 — and land behind the fetching wave's own waits (the epilogue: vmcnt(7), then vmcnt(0)). Every
    // wave fetches the rows of ITS OWN 80 x 64 block, as pieces of 16 rows x 64 bytes (32 columns): lane l reads 16 bytes of row
    // l >> 2, chunk (l & 3) ^ (l >> 4) — the four rows that share a 64-byte quarter of the 256-byte bank row hold a column chunk
    // at four different places, so the epilogue's 8-byte reads in the accumulator layout (16 rows x 2 half chunks per 32 lanes)
    // touch every bank once. Piece (j, h) = row block j of five, column half h. The six operations that all eight waves issue as
    // 16-byte pieces carry, in issue order (A, A, W0, W0, W1, W1): first staging (0,0) (0,1) (1,0) (1,1) (2,0) (2,1), second
    // staging — ko2 = two row blocks on — (2,.) again, (3,0) (3,1) (4,0) (4,1). The third A operation (a piece on waves 0-3, the
    // 4-byte filler on 4-7) re-reads piece (0,0) / (2,0): inside the tile like everything else, read by nobody.
    const int rblk = 16 * ep.ldo * 2;           // bytes between two row blocks of the output
    const int lane_vo_r = ((lane >> 2) * ep.ldo + (((lane & 3) ^ (lane >> 4)) * 8)) * 2;
// after a K-tile's stagings: the next K-tile to stage, or (residual GEMMs) the old rows in place of K-tiles nt and nt + 1
#define G160_NEXT_KTILE()                                                                                    \
    if (++k2 == nt) {                                                                                       \
        if constexpr (RESID) {                                                                              \
            srdA = srdW = __builtin_amdgcn_make_buffer_rsrc(                                                \
                reinterpret_cast<uint16_t*>(ep.out) + (size_t)(bm * 160 + wm * 80) * ep.ldo + bn * 256 + wn * 64, 0, 0x7fffffff, \
                0x00020000);                                                                                \
            lane_vo = lane_vo_r;                                                                            \
            xa0 = 0; xa1 = 64; xa2 = 0; xaf = 0;                                                            \
            xw0 = rblk; xw1 = rblk + 64; xw2 = 2 * rblk; xw3 = 2 * rblk + 64;                               \
            ko2 = 0; kstep = 2 * rblk;                                                                      \
        } else { k2 = 0; ko2 = 0; }                                                                         \
    } else { ko2 += kstep; }

    // ---- PIX: the A slot from the f32 pixels. Piece j of this wave (rows 8 (wave + 8 j) + r_in; waves 4-7 have no third piece
    // and fetch their second one again, unused, so that every wave issues six loads per K-tile) at per-lane byte offset pvo[j]
    // = pixel (img, c = 0, py * P + dky, px * P + kx) of its row's patch, dky / kx = where chunk p lies in the K-tile's
    // 64 / P pixel-row segments; K-tile kt adds the scalar offset of (c, ky0). Pad rows read the last valid row's patch.
    u32x4 srdP = {0u, 0u, 0u, 0u};
    int pvo[3] = {0, 0, 0};
    u32x4 pa[2][6];
    int pix_S = 0, pix_tshift = 0, pix_rows = 0, pix_half = 0;
    if constexpr (PIX) {
        const uint64_t a64 = (uint64_t)A;
        srdP = u32x4{(uint32_t)a64, (uint32_t)(a64 >> 32) & 0xffffu, (uint32_t)ep.pix_bytes, 0x00020000u};
        const int S = ep.pix_S, P = ep.pix_P, G = S / P, GG = ep.p0;
        pix_S = S;
        pix_tshift = P == 32 ? 4 : 2;   // K-tiles per channel = P * P / 64
        pix_rows = 64 / P;              // pixel rows per K-tile
        // a lane's two loads are floats 4 p .. 4 p + 3 of the K-tile's first and second 32: eight lanes read 128 contiguous
        // bytes of one patch row (P = 32: one pixel-row segment; P = 16: two of 64 bytes)
        const int dky = P == 32 ? 0 : (p >> 2), kx = P == 32 ? p * 4 : (p & 3) * 4;
        pix_half = (P == 32 ? 1 : 2) * S * 4;   // bytes from the first 32 floats of a K-tile to the second
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int q = wave + 8 * ((j == 2 && wave >= 4) ? 1 : j);
            int m = bm * 160 + q * 8 + r_in;
            m = m < ep.m_valid ? m : ep.m_valid - 1;
            const int img = m / GG, pr = m - img * GG, py = pr / G, px = pr - py * G;
            pvo[j] = (((img * 3) * S + py * P + dky) * S + px * P + kx) * 4;
        }
    }
// six loads of K-tile kt into register set `set` (not counted by the compiler: G160_PIX_WRITE's wait names them)
#define G160_PIX_LOAD(set, kt)                                                                               \
    {                                                                                                       \
        const int c_ = (kt) >> pix_tshift;                                                                  \
        const int so_ = (c_ * pix_S + ((kt) - (c_ << pix_tshift)) * pix_rows) * pix_S * 4;                  \
        const int so2_ = so_ + pix_half;                                                                    \
        _Pragma("unroll") for (int j = 0; j < 3; ++j)                                                       \
            asm volatile("buffer_load_dwordx4 %0, %2, %3, %4 offen\n\tbuffer_load_dwordx4 %1, %2, %3, %5 offen" \
                         : "=&v"(pa[set][2 * j]), "=&v"(pa[set][2 * j + 1])                                 \
                         : "v"(pvo[j]), "s"(srdP), "s"(so_), "s"(so2_)                                      \
                         : "memory");                                                                       \
    }
// register set `set` has landed once at most `cnt` younger operations are in flight: convert, write the A slot of buffer b2
#define G160_PIX_WRITE(set, b2, cnt)                                                                         \
    {                                                                                                       \
        asm volatile("s_waitcnt vmcnt(" #cnt ")"                                                            \
                     : "+v"(pa[set][0]), "+v"(pa[set][1]), "+v"(pa[set][2]), "+v"(pa[set][3]), "+v"(pa[set][4]), "+v"(pa[set][5]) \
                     :: "memory");                                                                          \
        /* floats 4 p .. of the first 32 are half (p & 1) of chunk p >> 1, of the second 32 of chunk 4 + (p >> 1) */ \
        const int ao_ = (b2) * G160_BUF + a_dst + r_in * 128 + (((p >> 1) ^ r_in) << 4) + ((p & 1) << 3);   \
        _Pragma("unroll") for (int j = 0; j < 3; ++j) {                                                     \
            const u32x4 lo_ = pa[set][2 * j], hi_ = pa[set][2 * j + 1];                                     \
            u32x2 pl_, ph_;                                                                                 \
            pl_[0] = pack_bf16x2(__uint_as_float(lo_[0]), __uint_as_float(lo_[1]));                         \
            pl_[1] = pack_bf16x2(__uint_as_float(lo_[2]), __uint_as_float(lo_[3]));                         \
            ph_[0] = pack_bf16x2(__uint_as_float(hi_[0]), __uint_as_float(hi_[1]));                         \
            ph_[1] = pack_bf16x2(__uint_as_float(hi_[2]), __uint_as_float(hi_[3]));                         \
            if (j < 2 || wave < 4) {                                                                        \
                *reinterpret_cast<u32x2*>(smem + ao_ + j * 8 * 1024) = pl_;                                 \
                *reinterpret_cast<u32x2*>(smem + (ao_ ^ 64) + j * 8 * 1024) = ph_;                          \
            }                                                                                               \
        }                                                                                                   \
    }

    // ---- fragment reads: one base per operand and k step + immediate (buffer, 16-row block)
    uint32_t ab[2], wb[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const uint32_t sw = (((4 * s + fg) ^ (fr & 7)) << 4);
        ab[s] = (wm * 80 + fr) * 128 + sw;
        wb[s] = G160_A_BYTES + (wn * 32 + fr) * 128 + sw;
    }
    frag am[5];
    frag wq[4];
    f32x4 acc[4][5];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 5; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

// the fragments of k step s (32 of the K-tile's 64 columns): five A row blocks, four W column blocks (n0: 0, 1; n1: 2, 3)
#define G160_READ(b, s)                                                                                      \
    {                                                                                                       \
        _Pragma("unroll") for (int mf = 0; mf < 5; ++mf)                                                    \
            am[mf] = *reinterpret_cast<const frag*>(smem + ab[s] + (b) * G160_BUF + mf * 2048);             \
        _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                       \
            wq[i] = *reinterpret_cast<const frag*>(smem + wb[s] + (b) * G160_BUF + (i >> 1) * G160_W_BYTES + (i & 1) * 2048); \
    }
// the 20 MFMAs of one phase: all five row blocks against all four column blocks, one k step
#define G160_MMA()                                                                                           \
    {                                                                                                       \
        __builtin_amdgcn_s_setprio(1);                                                                      \
        _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                       \
            _Pragma("unroll") for (int mf = 0; mf < 5; ++mf)                                                \
                acc[i][mf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wq[i], am[mf], acc[i][mf], 0, 0, 0);   \
        __builtin_amdgcn_s_setprio(0);                                                                      \
    }
// (p256s_barrier, p256s_late_reads_done: gemm_p256_stream.h. The half that runs one barrier behind reads a buffer for the last
// time in the interval right before the other half restages it.)
// K-tile t out of buffer B while K-tile t+2 (byte offset ko2) is staged into buffer B2 = (B + 2) % 3, which held K-tile t-1.
// The two phases are the two K STEPS of the tile (32 columns each): every read part pulls 9 fragments (5 A + 4 W) and every
// MFMA part is the full 5 x 4 block. A wave issues 7 LDS-DMA operations per K-tile (A A A in phase 0, W0 W0 W1 W1 in phase
// 1). All three slots of a K-tile are read from its phase 0 on: the one wait, in phase 1, retires K-tile t+1 completely —
// younger than it are exactly K-tile t+2's seven: vmcnt(7). Both halves' waits and a barrier precede both halves' reads of
// what they retire.
#define G160_KTILE(B, B2)                                                                                    \
    {                                                                                                       \
        G160_READ(B, 0);                                                                                    \
        G160_STAGE_A(B2, ko2);                                                                              \
        p256s_late_reads_done(wm);                                                                             \
        p256s_barrier();                                                                                     \
        G160_MMA();                                                                                         \
        p256s_barrier();                                                                                     \
        G160_READ(B, 1);                                                                                    \
        G160_STAGE_W(B2, 0, ko2);                                                                           \
        G160_STAGE_W(B2, 1, ko2);                                                                           \
        p256s_late_reads_done(wm);                                                                             \
        asm volatile("s_waitcnt vmcnt(7)" ::: "memory");                                                    \
        p256s_barrier();                                                                                     \
        G160_MMA();                                                                                         \
        p256s_barrier();                                                                                     \
        G160_NEXT_KTILE();                                                                                  \
    }

// PIX, K-tile t (even / odd: SET = 0 / 1) out of buffer B: phase 0 requests K-tile t + 2's pixels into set SET, phase 1 converts
// K-tile t + 1's (set SET ^ 1, requested a K-tile and a half ago; younger: K-tile t + 1's four W pieces and the six loads just
// issued) into the A slot of buffer B1 = (B + 1) % 3 — last read during K-tile t - 2, first read after this phase's barriers
// on either wave half — and stages K-tile t + 2's W slots by LDS-DMA as ever. The closing wait retires K-tile t + 1's W pieces
// (younger: six loads and four pieces of K-tile t + 2) and every wave's LDS writes.
#define G160_KTILE_PIX(B, B1, B2, SET)                                                                       \
    {                                                                                                       \
        G160_READ(B, 0);                                                                                    \
        G160_PIX_LOAD(SET, k2);                                                                             \
        p256s_late_reads_done(wm);                                                                             \
        p256s_barrier();                                                                                     \
        G160_MMA();                                                                                         \
        p256s_barrier();                                                                                     \
        G160_READ(B, 1);                                                                                    \
        G160_PIX_WRITE((SET) ^ 1, B1, 10);                                                                  \
        G160_STAGE_W(B2, 0, ko2);                                                                           \
        G160_STAGE_W(B2, 1, ko2);                                                                           \
        asm volatile("s_waitcnt vmcnt(10) lgkmcnt(0)" ::: "memory");                                        \
        p256s_barrier();                                                                                     \
        G160_MMA();                                                                                         \
        p256s_barrier();                                                                                     \
        G160_NEXT_KTILE();                                                                                  \
    }

    // ---- this wave's bias values (1 KB per workgroup): requested NOW, in front of the prologue's LDS-DMA, so that the epilogue
    // of this one-tile workgroup starts without a memory round trip
    f32x4 bias[4];
    if constexpr (RESID) {
#pragma unroll
        for (int i = 0; i < 4; ++i) bias[i] = *reinterpret_cast<const f32x4*>(ep.bias + bn * 256 + wn * 64 + i * 16 + 4 * fg);
    }

    // prologue: K-tiles 0 and 1 into buffers 0 and 1 (14 operations per wave)
    int ko2 = 0, k2 = 2;
    if constexpr (PIX) {   // 20 operations: K-tile 0's pixels are converted here, K-tile 1's in phase 1 of K-tile 0
        G160_PIX_LOAD(0, 0);
        G160_STAGE_W(0, 0, 0);
        G160_STAGE_W(0, 1, 0);
        G160_PIX_LOAD(1, 1);
        G160_STAGE_W(1, 0, GEMM_BK * 2);
        G160_STAGE_W(1, 1, GEMM_BK * 2);
        G160_PIX_WRITE(0, 0, 14);   // (younger than K-tile 0's loads: 4 + 6 + 4)
        ko2 = 2 * GEMM_BK * 2;
        asm volatile("s_waitcnt vmcnt(10) lgkmcnt(0)" ::: "memory");  // K-tile 0's W pieces (younger: K-tile 1's ten), the A writes
    } else {
    G160_STAGE_A(0, 0);
    G160_STAGE_W(0, 0, 0);
    G160_STAGE_W(0, 1, 0);
    G160_STAGE_A(1, GEMM_BK * 2);
    G160_STAGE_W(1, 0, GEMM_BK * 2);
    G160_STAGE_W(1, 1, GEMM_BK * 2);
    ko2 = (nt > 2) ? 2 * GEMM_BK * 2 : 0;   // (K >= 256: nt >= 4)
    asm volatile("s_waitcnt vmcnt(7)" ::: "memory");  // K-tile 0 has landed (younger: K-tile 1's seven)
    }
    // ... and with it the four bias loads above, which are older: their round trip ran beside the prologue's. Pinned here
    // so that the compiler's own wait for them sits in front of the K loop, not inside it.
    if constexpr (RESID) {
#pragma unroll
        for (int i = 0; i < 4; ++i) asm volatile("" : "+v"(bias[i]));
    }
    p256s_barrier();
    if (wm == 1) p256s_barrier();  // the lower half runs one barrier behind from here on

    if constexpr (PIX) {
#pragma unroll 1   // three buffers x two register sets: nt % 6 == 0 (12 K-tiles at P = 16, 48 at P = 32)
        for (int t = 0; t < nt; t += 6) {
            G160_KTILE_PIX(0, 1, 2, 0);
            G160_KTILE_PIX(1, 2, 0, 1);
            G160_KTILE_PIX(2, 0, 1, 0);
            G160_KTILE_PIX(0, 1, 2, 1);
            G160_KTILE_PIX(1, 2, 0, 0);
            G160_KTILE_PIX(2, 0, 1, 1);
        }
    } else {
#pragma unroll 1   // (nt may be a compile-time constant, KT: the loop stays a loop — one copy of the K-tile triple)
    for (int t = 0; t < nt; t += 3) {
        G160_KTILE(0, 2);
        if (t + 1 < nt) G160_KTILE(1, 0);
        if (t + 2 < nt) G160_KTILE(2, 1);
    }
    }
    if (wm == 0) p256s_barrier();   // (the upper half's last barrier: the lower half is still one behind)

    if constexpr (PATCH) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the last two stagings (wrap-around) have landed ...
        p256s_barrier();                // ... on every wave, and every wave has read its last fragments: the buffers are free
        // f32 rows: 16 rows x 32 columns at a time through the wave's 2 KB patch (16-byte chunks XOR-swizzled by the row), read back
        // as whole 128-byte row segments; patch row m of the GEMM is token 1 + m % p0 of item m / p0, the position row is added
        int lane_e = lane;
        asm volatile("" : "+v"(lane_e));
        const int efr = lane_e & 15, efg = lane_e >> 4;
        const int rrow = lane_e >> 3, rchunk = lane_e & 7;
        char* patch = smem + wave * 2048;   // (buffer 0)
        float* outp = reinterpret_cast<float*>(ep.out);
#pragma unroll
        for (int j = 0; j < 5; ++j) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
#pragma unroll
                for (int ii = 0; ii < 2; ++ii)
                    *reinterpret_cast<f32x4*>(patch + efr * 128 + (((ii * 4 + efg) ^ (efr & 7)) << 4)) = acc[2 * h + ii][j];
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
                for (int rh = 0; rh < 2; ++rh) {
                    const int row = rh * 8 + rrow;
                    const f32x4 v = *reinterpret_cast<const f32x4*>(patch + row * 128 + ((rchunk ^ (row & 7)) << 4));
                    const int m = bm * 160 + wm * 80 + j * 16 + row;
                    const int n = bn * 256 + wn * 64 + h * 32 + rchunk * 4;
                    if (m < ep.m_valid) {
                        const int img = m / ep.p0, pt = m - img * ep.p0;
                        const f32x4 pos = *reinterpret_cast<const f32x4*>(ep.aux + (size_t)(1 + pt) * ep.ldo + n);
                        *reinterpret_cast<f32x4*>(outp + ((size_t)img * ep.p1 + 1 + pt) * ep.ldo + n) = v + pos;
                    }
                }
                __builtin_amdgcn_wave_barrier();  // the patch is rewritten by the next half
            }
        }
    }
    // ---- epilogue of MMISS_EPI_BIAS_RESID_BF16 (gemm_bf16.h gemm_epilogue: same arithmetic, same statistics, bit for bit),
    // per wave: 5 row blocks x 64 columns through the wave's two 2 KB transpose patches, whole 128-byte row segments per store.
    //
    // What a block reads of the old rows, and who fetched it (G160_NEXT_KTILE, G160_STAGE_A / _W): block 0 = pieces (0,0), (0,1)
    // = the first two A operations of the FIRST late staging, at a_dst and a_dst + 8 KB of buffer nt % 3; blocks 1 and 2 =
    // that staging's W n0 / W n1 operations, at w_dst and w_dst + 1 KB of the two W slots; blocks 3 and 4 = the W n0 / W n1
    // operations of the SECOND staging, same places in buffer (nt + 1) % 3. a_dst and w_dst are the wave's own: a wave reads
    // only pieces it issued itself, so its own counted wait is all it needs. The K loop's last wait (vmcnt(7), phase 1 of
    // K-tile nt - 1) has already retired the first staging; blocks 0..2 start behind it and the barrier that frees the last
    // fragment buffer, while the second staging's seven operations are still in flight. The wait for those, vmcnt(0), stands
    // in front of the wave's FIRST output store: stores count in vmcnt too and are not ordered against loads, so no counted
    // wait could be had behind one.
    if constexpr (RESID) {
        int lane_e = lane;
        asm volatile("" : "+v"(lane_e));
        const int efr = lane_e & 15, efg = lane_e >> 4;
        const int rrow = lane_e >> 3, rchunk = lane_e & 7;
        // the old rows, out of the slots the last two stagings filled, in the accumulator layout: 8 bytes per lane and 16 x 16 block
        u32x2 resid[5][4];
        const char* const st0 = smem + (nt % 3) * G160_BUF;         // the staging issued during K-tile nt - 2
        const char* const st1 = smem + ((nt + 1) % 3) * G160_BUF;   // ... during K-tile nt - 1
        const int rd = efr * 64 + ((((efg >> 1) ^ (efr >> 2)) << 4) | ((efg & 1) << 3));
#define G160_OLD_ROWS(j)                                                                                     \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                         \
        const int h = i >> 1;                                                                               \
        const char* piece = (j) == 0 ? st0 + a_dst + h * 8 * 1024                                           \
                                     : ((j) < 3 ? st0 : st1) + G160_A_BYTES + (((j) - 1) & 1) * G160_W_BYTES + w_dst + h * 1024; \
        resid[j][i] = *reinterpret_cast<const u32x2*>(piece + (rd ^ ((i & 1) << 5)));                       \
    }
        asm volatile("s_waitcnt vmcnt(7)" ::: "memory");   // the first late staging has landed (younger: the second one's seven)
        G160_OLD_ROWS(0);
        G160_OLD_ROWS(1);
        G160_OLD_ROWS(2);
        p256s_barrier();   // every wave has read its last fragments: buffer (nt - 1) % 3, which no late staging fills, is free
        // two patches per wave, blocks alternate: block j + 1 is written while block j's read-back is on its way
        char* const patch = smem + ((nt + 2) % 3) * G160_BUF + wave * 4096;
        // a lane's four packed writes of a block (row efr, 8-byte unit (4 i + efg) ^ 2 (efr & 7)) and its two 16-byte reads
        // (rows rrow and 8 + rrow, chunk rchunk ^ rrow): per-lane offsets fixed for the tile, block and half are immediates
        const int wr0 = efr * 128 + ((efg ^ (2 * (efr & 7))) << 3);
        const int wr[4] = {wr0, wr0 ^ 32, wr0 ^ 64, wr0 ^ 96};
        const int rdp = rrow * 128 + ((rchunk ^ rrow) << 4);
        // output rows: the lane's 16 bytes of rows row0 + rrow + 8 k, k = 0..9; row k is valid while 8 k < lim, every other
        // one goes to the dump row M - 1
        const int row0 = bm * 160 + wm * 80, col0 = bn * 256 + wn * 64;
        const __amdgpu_buffer_rsrc_t srdO = __builtin_amdgcn_make_buffer_rsrc(ep.out, 0, 0x7fffffff, 0x00020000);
        const int vo0 = ((row0 + rrow) * ep.ldo + col0 + rchunk * 8) * 2;
        const int vo_dump = ((M - 1) * ep.ldo + col0 + rchunk * 8) * 2;
        const int ostep = 8 * ep.ldo * 2;
        const int lim = ep.m_valid - row0 - rrow;
        // statistics [row][ldo / 64][2]: a descriptor that ends with the last valid row (no records without stats_out) drops
        // the pad rows' stores, and the seven lanes of a row that do not store start beyond any record. Deliberately without
        // a branch on stats_out: without statistics the sums are still computed and their ten stores dropped by the empty
        // descriptor (not timed: the headline step's 22 launches all ask for statistics), which keeps the epilogue one straight line
        const int mv = ep.m_valid < M ? ep.m_valid : M;
        const __amdgpu_buffer_rsrc_t srdS =
            __builtin_amdgcn_make_buffer_rsrc(ep.stats_out, 0, ep.stats_out ? mv * (ep.ldo >> 6) * 8 : 0, 0x00020000);
        const int so0 = rchunk == 0 ? ((row0 + rrow) * (ep.ldo >> 6) + (col0 >> 6)) * 8 : (int)0x80000000u;
        const int sstep = 8 * (ep.ldo >> 6) * 8;
// block j: old rows + product + bias, rounded, packed, into patch j & 1
#define G160_BLOCK(j)                                                                                        \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                         \
        const f32x4 v = acc[i][j] + bias[i];                                                                \
        float y[4];                                                                                         \
        y[0] = __uint_as_float(resid[j][i][0] << 16) + v[0];                                                \
        y[1] = __uint_as_float(resid[j][i][0] & 0xFFFF0000u) + v[1];                                        \
        y[2] = __uint_as_float(resid[j][i][1] << 16) + v[2];                                                \
        y[3] = __uint_as_float(resid[j][i][1] & 0xFFFF0000u) + v[3];                                        \
        u32x2 pk;                                                                                           \
        pk[0] = pack_bf16x2(y[0], y[1]);                                                                    \
        pk[1] = pack_bf16x2(y[2], y[3]);                                                                    \
        *reinterpret_cast<u32x2*>(patch + ((j) & 1) * 2048 + wr[i]) = pk;                                   \
    }
        G160_BLOCK(0);
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            // block j's writes before its reads; block j - 1's reads before block j + 1's writes (the same patch)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            u32x4 pk[2];
#pragma unroll
            for (int rh = 0; rh < 2; ++rh) pk[rh] = *reinterpret_cast<const u32x4*>(patch + (j & 1) * 2048 + rh * 1024 + rdp);
            if (j == 0) { G160_BLOCK(1); }
            if (j == 1) { G160_BLOCK(2); }
            if (j == 2) { G160_BLOCK(3); }
            if (j == 3) { G160_BLOCK(4); }
            if (j == 0) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the second late staging has landed (no store issued yet)
                G160_OLD_ROWS(3);
                G160_OLD_ROWS(4);
            }
            // rows 2 j and 2 j + 1 of the lane's ten, and the statistics of what was STORED (the rounded rows are the residual
            // stream from here on)
            float rs[2], rq[2];
#pragma unroll
            for (int rh = 0; rh < 2; ++rh) {
                const int k = 2 * j + rh;
                // sc1: written through. All 240 workgroups store their 80 KB at the same time and end right after; plain
                // stores leave all of it dirty in the L2s for the write-back at the kernel's end, these go out while the
                // other waves still compute (profiles/gemm_p160_epilogue.txt, section 3: isolated, out-projection 19.5 ->
                // 18.1 us, FC2 51.8 -> 51.0, nt stores no gain; the step 2.621 -> 2.592 ms). The persistent 256 x 256 kernel,
                // whose stores are spread over its run, found the three policies equal (profiles/gemm_p256_r03.txt)
                __builtin_amdgcn_raw_buffer_store_b128(pk[rh], srdO, 8 * k < lim ? vo0 + k * ostep : vo_dump, 0, 16);
                g160_row_part(pk[rh], rs[rh], rq[rh]);
            }
            g160_row_sum8(rs[0], rq[0], rs[1], rq[1]);
#pragma unroll
            for (int rh = 0; rh < 2; ++rh)
                __builtin_amdgcn_raw_buffer_store_b64(u32x2{__float_as_uint(rs[rh]), __float_as_uint(rq[rh])}, srdS,
                                                      so0 + (2 * j + rh) * sstep, 0, 0);
        }
#undef G160_OLD_ROWS
#undef G160_BLOCK
    }
}
#undef G160_BLDS
#undef G160_FILL
#undef G160_STAGE_A
#undef G160_STAGE_W
#undef G160_READ
#undef G160_MMA
#undef G160_KTILE
#undef G160_KTILE_PIX
#undef G160_PIX_LOAD
#undef G160_PIX_WRITE
#undef G160_NEXT_KTILE
#undef G160_X

// can the residual GEMM on the bf16 stream run on this tile? (the tile must divide the padded rows / the columns; 32-bit offsets)
static inline bool gemm160p_ok(int M, int N, int K) {
    if (M <= 0 || (M % 160) || N <= 0 || (N % 256) || K < 256 || (K % 128)) return false;
    if ((int64_t)M * N * 2 >= (1LL << 31) || (int64_t)160 * K * 2 >= (1LL << 31) || (int64_t)256 * K * 2 >= (1LL << 31)) return false;
    return true;
}

// out (bf16 [M, ldo], in place) = bf16(f32(out) + A W^T + bias), ep.stats_out optional; M padded to 160 (rows >= ep.m_valid land
// in row M - 1)
static int launch_gemm160p(hipStream_t st, const void* A, const void* W, const GemmEpi& ep, int M, int N, int K) {
    if (!gemm160p_ok(M, N, K)) MM_FAIL(MMISS_ERR_UNSUPPORTED, "gemm160p: M=%d N=%d K=%d", M, N, K);
    if (!ep.out || !ep.bias || ep.ldo < N || (ep.ldo % 64)) MM_FAIL(MMISS_ERR_ARG, "gemm160p: missing operand");
    const int mv = ep.m_valid < M ? ep.m_valid : M;
    const double bytes = 2.0 * ((double)mv * K + (double)N * K) + 2.0 * 2.0 * (double)mv * N;
    char pname[48];
    snprintf(pname, sizeof(pname), "gemm_bf16_bias_resid16_p160_k%d", K);
    MM_PROF(pname, st, 2.0 * mv * N * K, bytes);
#define G160_KT_CASE(KT_)                                                                                                        \
    if (K == (KT_) * GEMM_BK) {                                                                                                  \
        MM_TRY(mmiss_ensure_dyn_lds(reinterpret_cast<const void*>(&gemm160p_kernel<MMISS_EPI_BIAS_RESID_BF16, KT_>), G160_LDS)); \
        hipLaunchKernelGGL((gemm160p_kernel<MMISS_EPI_BIAS_RESID_BF16, KT_>), dim3((M / 160) * (N / 256)), dim3(512), G160_LDS, \
                           st, reinterpret_cast<const __bf16*>(A), reinterpret_cast<const __bf16*>(W), M, N, K, ep);            \
        MM_HIP(hipGetLastError());                                                                                              \
        return MMISS_OK;                                                                                                        \
    }
    // the towers' shapes: ViT-B/32 out-projection / FC2 (768, 3072), its text tower (512, 2048), ViT-L/14 (1024, 4096)
    G160_KT_CASE(12) G160_KT_CASE(48) G160_KT_CASE(8) G160_KT_CASE(32) G160_KT_CASE(16) G160_KT_CASE(64)
#undef G160_KT_CASE
    MM_TRY(mmiss_ensure_dyn_lds(reinterpret_cast<const void*>(&gemm160p_kernel<MMISS_EPI_BIAS_RESID_BF16>), G160_LDS));
    hipLaunchKernelGGL((gemm160p_kernel<MMISS_EPI_BIAS_RESID_BF16>), dim3((M / 160) * (N / 256)), dim3(512), G160_LDS, st, reinterpret_cast<const __bf16*>(A),
                       reinterpret_cast<const __bf16*>(W), M, N, K, ep);
    MM_HIP(hipGetLastError());
    return MMISS_OK;
}

// The patch-embedding GEMM (MMISS_EPI_PATCH_F32 of gemm_bf16.h: ep.out f32 [items * p1, ldo], ep.aux = position table, ep.p0 = patches
// per item, ep.p1 = tokens per item) on the same tile: 12 544 patch rows x 768 x 3072 at bs 256 = 79 x 3 tiles.
static int launch_gemm160p_patch(hipStream_t st, const void* A, const void* W, const GemmEpi& ep, int M, int N, int K) {
    if (!gemm160p_ok(M, N, K)) MM_FAIL(MMISS_ERR_UNSUPPORTED, "gemm160p_patch: M=%d N=%d K=%d", M, N, K);
    if (!ep.out || !ep.aux || ep.p0 <= 0 || ep.p1 <= 0 || ep.ldo < N) MM_FAIL(MMISS_ERR_ARG, "gemm160p_patch: missing operand");
    const int mv = ep.m_valid < M ? ep.m_valid : M;
    MM_PROF("gemm_bf16_patch_p160", st, 2.0 * mv * N * K, 2.0 * ((double)mv * K + (double)N * K) + 4.0 * (double)mv * N);
    MM_TRY(mmiss_ensure_dyn_lds(reinterpret_cast<const void*>(&gemm160p_kernel<MMISS_EPI_PATCH_F32>), G160_LDS));
    hipLaunchKernelGGL((gemm160p_kernel<MMISS_EPI_PATCH_F32>), dim3((M / 160) * (N / 256)), dim3(512), G160_LDS, st,
                       reinterpret_cast<const __bf16*>(A), reinterpret_cast<const __bf16*>(W), M, N, K, ep);
    MM_HIP(hipGetLastError());
    return MMISS_OK;
}

// The same GEMM with the A operand read straight from the f32 pixels [B,3,S,S] (no im2col pass): K = 3 P^2, P = 16 or 32,
// ep.p0 = (S / P)^2 patches per item. The same bits as im2col + launch_gemm160p_patch. The class's bytes name the pixels.
static inline bool gemm160p_pix_ok(const void* pixels, int B, int S, int P, int M, int N, int K) {
    if (!(P == 16 || P == 32) || S <= 0 || (S % P) || K != 3 * P * P || !gemm160p_ok(M, N, K)) return false;
    const int G = S / P;
    if ((int64_t)B * G * G > M || ((uintptr_t)pixels & 15)) return false;
    return (int64_t)B * 3 * S * S * 4 < (1LL << 31);   // 32-bit byte offsets into the image
}
static int launch_gemm160p_patch_pix(hipStream_t st, const void* pixels, const void* W, const GemmEpi& ep0, int B, int S, int P, int M,
                                     int N, int K) {
    if (!gemm160p_pix_ok(pixels, B, S, P, M, N, K)) MM_FAIL(MMISS_ERR_UNSUPPORTED, "gemm160p_patch_pix: B=%d S=%d P=%d M=%d N=%d K=%d", B, S, P, M, N, K);
    GemmEpi ep = ep0;
    const int G = S / P;
    if (!ep.out || !ep.aux || ep.p0 != G * G || ep.p1 <= 0 || ep.ldo < N || ep.m_valid != B * G * G)
        MM_FAIL(MMISS_ERR_ARG, "gemm160p_patch_pix: missing operand");
    ep.pix_S = S; ep.pix_P = P; ep.pix_bytes = (int)((int64_t)B * 3 * S * S * 4);
    const int mv = ep.m_valid;
    MM_PROF("gemm_bf16_patch_p160", st, 2.0 * mv * N * K, 4.0 * (double)B * 3 * S * S + 2.0 * (double)N * K + 4.0 * (double)mv * N);
    MM_TRY(mmiss_ensure_dyn_lds(reinterpret_cast<const void*>(&gemm160p_kernel<MMISS_EPI_PATCH_PIX_F32>), G160_LDS));
    hipLaunchKernelGGL((gemm160p_kernel<MMISS_EPI_PATCH_PIX_F32>), dim3((M / 160) * (N / 256)), dim3(512), G160_LDS, st,
                       reinterpret_cast<const __bf16*>(pixels), reinterpret_cast<const __bf16*>(W), M, N, K, ep);
    MM_HIP(hipGetLastError());
    return MMISS_OK;
}
