// gemm_p256_stream.h — the K-tile stream of the persistent 256x256 GEMMs, once: gemm256p_kernel (gemm_bf16_p256.h),
// gemm256s_kernel (gemm_strip_p256.h) and gemm256p8_kernel (gemm_fp8_p256.h) run one workgroup per CU over its tiles as ONE
// continuous stream of K-tiles — staggered wave halves, four phases per K-tile, LDS-DMA staging with scalar offsets, counted
// waits (the why: head of gemm_bf16_p256.h). Included by gemm_bf16_256.h behind its G256_SLOT, the size of a staging slot;
// gemm256_kernel and gemm160p_kernel take the two barrier helpers from here and nothing else.
//
// FUNCTIONS: the barrier, the late half's read fence, the two LDS-DMA forms and tile_of — the machine code of every kernel
// is the same with them as with the macros they replace.
// MACROS (P256S_*), and why:
//   * staging, the K-tile, the pair, the prologue, the tile driver read and move the kernel's stream state (oA1, oW1, mA1,
//     oA2, oW2, k2, cbm, cbn, chalf) and call its hooks and its lambdas (epilogue, stage_x). They bind to those and to smem,
//     wave, wm, stage_dst, a_vo, w_vo, row8, srdA, srdW, nfull, nhalf, mine, npair by name: as functions they would take the
//     state by reference (the attention refactor found that filling reference parameters changes registers and waits), and
//     the hooks are macros of the kernel's own locals;
//   * the tile list (P256S_BUILD_TILE_LIST over P256_DEAL_RULE / P256_ENTRY_RULE of p256_deal.h): as an inlined function
//     returning the deal the same values were computed in another order, which moved instructions in front of the K loop
//     of every gemm256p_kernel (profiles/p256_stream_refactor.txt);
//   * the slot map, the 16-bit fragment reads and MFMA block: used inside address immediates / over the kernel's register arrays.
//
// HOOKS: what a kernel defines immediately before its body and undefines behind it:
//   KT_READ_A(b, mq), KT_READ_W(b, nq)   fragment reads of A slot mq / W slot nq of buffer b
//   KT_MMA(mq, nq)                       the MFMA block of quadrant (mq, nq)
//   KT_STAGE_W(dst, which, b, oW)        staging of W slot `which` (2, 3): P256S_STAGE_W, or the strip kernel's fp8 form
//   KT_WAIT(POST, b, which)              the counted wait `which` (0, 1, 3) of a K-tile out of buffer b
//   KT_PHASE3(FIN)                       extra work of the last, read-free phase
//   KT_ADVANCE()                         move the stream positions t+1 / t+2 on by one K-tile
//   KT_PAIR_HEAD(kp), KT_AFTER_EPILOGUE() the tile driver's two hooks (P256S_RUN_TILES)
#pragma once
#include "gemm_bf16.h"
#include "p256_deal.h"

// ---- the slot map. LDS slot order: A m0 (buffer 0, 1), A m1 (0, 1), W n0 (0, 1), W n1 (0, 1), so that ONE base register per
// operand and k step reaches every slot of the operand with a 16-bit immediate. which: 0 = A m0, 1 = A m1, 2 = W n0, 3 = W n1.
// Slot row r of an A slot is the activation row (r>>6)*128 + mq*64 + (r&63) of the tile, of a W slot the weight row
// (r>>5)*64 + nq*32 + (r&31); a wave stages slot rows 16*wave .. 16*wave+15 as two 8-row pieces of 128-byte rows.
#define P256S_SLOT(which, b) (((which) * 2 + (b)) * G256_SLOT)

// ---- LDS-DMA, buffer form: per-lane byte offset vo computed once (ONE VGPR per operand), everything else — tile, K-tile,
// m / n half, 8-row piece — in the scalar offset so. 16 or 4 bytes per lane.
// (default cache policy, aux = 0: nt operand loads measured 5-12 % slower on either operand, sc0 / sc1 equal; round 4)
// (arguments in the builtin's order: the destination is evaluated in front of the offsets, as it was when these were macros)
__device__ __forceinline__ void p256s_blds16(__amdgpu_buffer_rsrc_t srd, char* dst, int vo, int so) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(srd, (__attribute__((address_space(3))) void*)(dst), 16, vo, so, 0, 0);
}
__device__ __forceinline__ void p256s_blds4(__amdgpu_buffer_rsrc_t srd, char* dst, int vo, int so) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(srd, (__attribute__((address_space(3))) void*)(dst), 4, vo, so, 0, 0);
}

// ---- the workgroup barrier of the phase loops: raw s_barrier (a __syncthreads() would drain the counted loads), fenced
// against the scheduler on both sides
__device__ __forceinline__ void p256s_barrier() {
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
}
// The slots the LATE half (wm = 1) reads in a phase are restaged by the early half right after the next barrier: its reads
// must have completed before that barrier (the early half's own reads complete a whole barrier earlier, with its MFMAs).
// (Free: 4096^3 101.8-104.1 us without it, 102.0-103.2 with it, round 3. Without it the order holds by timing only, not by construction.)
__device__ __forceinline__ void p256s_late_reads_done(int wm) {
    if (wm == 1) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

// ---- this workgroup's tile list (the deal: p256_deal.h), into the p256_table_entries entries at smem + TABLE.
// (decoded ONCE, in parallel, into LDS: the integer divisions are VALU code on this target, and inlined at the places of
// the unrolled K loop that move on to a next tile they pushed the kernel over its 256 registers: 233 spilled, 6 x slower)
// Declares nfull, nhalf and mine (P256_DEAL_RULE) in the kernel's scope; tid = the kernel's thread index.
#define P256S_BUILD_TILE_LIST(TABLE, nbm, nbn, m_fast)                                                       \
    const int T = (nbm) * (nbn), G = gridDim.x;                                                             \
    const int pb = xcd_remap(blockIdx.x, G);                                                                \
    P256_DEAL_RULE(T, G, pb)                                                                                \
    if (tid < mine && tid < p256_table_entries) {                                                           \
        P256_ENTRY_RULE(tid, G, pb)                                                                         \
        int bm_, bn_;                                                                                       \
        tile_order(L, nbm, nbn, m_fast, bm_, bn_);                                                          \
        reinterpret_cast<unsigned*>(smem + (TABLE))[tid] = P256_PACK(bm_, bn_, hf, P256_ENTRY_M1(pb));      \
    }                                                                                                       \
    __syncthreads();
__device__ __forceinline__ void p256s_tile_of(const char* table, int i, int& bm, int& bn, int& half) {
    // (an LDS-address-space load: through a generic pointer this was a flat_load + s_waitcnt vmcnt(0) — a drain of the
    // whole staging pipeline at every tile switch)
    const P256Tile t = p256_unpack((unsigned)__builtin_amdgcn_readfirstlane(((const __attribute__((address_space(3))) int*)table)[i]));
    bm = t.bm;
    bn = t.bn;
    half = t.half;
}

// ---- one slot's staging: both pieces are issued in the read part of the phase, behind its fragment reads. The second piece issued
// from the middle of the MFMA part instead measured 3-6 % SLOWER (round 3, 4096^3: 116-121 vs 111-113 us), the pieces issued
// BEFORE the fragment reads equal or slower (round 4): the read part is not what bounds the loop.
// LIVE = false: the slot is not read (the A m1 slot of a half tile): its two pieces shrink to 4 bytes per lane — the K
// stream is bound by LDS-DMA bytes per CU (64 KB per K-tile at ~40 GB/s), the operation COUNT must stay what the waits assume
// DST = where this wave's two pieces go: the loop forms it as (smem + slot) + stage_dst, the prologue as (smem + stage_dst) +
// slot (with one form for both, instructions of gemm256p_kernel in front of its K loop changed places and two instances
// changed their scalar spills).
#define P256S_STAGE_W(DST, which, oW, WROW8)                                                                 \
    {                                                                                                       \
        char* dst_ = (DST);                                                                                 \
        const int so_ = (oW) + ((which) & 1) * 4 * (WROW8);                                                 \
        p256s_blds16(srdW, dst_, w_vo, so_);                                                                \
        p256s_blds16(srdW, dst_ + 1024, w_vo, so_ + (WROW8));                                               \
    }
#define P256S_STAGE(which, b, oA, oW, LIVE) P256S_STAGE_TO(smem + P256S_SLOT(which, b) + stage_dst, which, b, oA, oW, LIVE)
#define P256S_STAGE_TO(DST, which, b, oA, oW, LIVE)                                                          \
    {                                                                                                       \
        if constexpr ((which) < 2) {                                                                        \
            char* dst_ = (DST);                                                                             \
            const int so_ = (oA);                                                                           \
            if (LIVE) {                                                                                     \
                p256s_blds16(srdA, dst_, a_vo, so_);                                                        \
                p256s_blds16(srdA, dst_ + 1024, a_vo, so_ + row8);                                          \
            } else {                                                                                        \
                p256s_blds4(srdA, dst_, a_vo, so_);                                                         \
                p256s_blds4(srdA, dst_ + 1024, a_vo, so_ + row8);                                           \
            }                                                                                               \
        } else {                                                                                            \
            KT_STAGE_W(DST, which, b, oW);                                                                  \
        }                                                                                                   \
    }

// ---- 16-bit operands (gemm256p_kernel, gemm256s_kernel's f16 rows): fragment reads — one base per operand and k step (ab[s],
// wb[s]) + immediate (slot, 16-row sub-tile) — and the MFMA block
#define P256S_READ_A16(b, mq)                                                                                \
    _Pragma("unroll") for (int mf = 0; mf < 4; ++mf) {                                                      \
        am[mf][0] = *reinterpret_cast<const frag*>(smem + ab[0] + P256S_SLOT(mq, b) + mf * 2048);           \
        am[mf][1] = *reinterpret_cast<const frag*>(smem + ab[1] + P256S_SLOT(mq, b) + mf * 2048);           \
    }
#define P256S_READ_W16(b, nq)                                                                                \
    _Pragma("unroll") for (int nf = 0; nf < 2; ++nf) {                                                      \
        wq[nq][nf][0] = *reinterpret_cast<const frag*>(smem + wb[0] + P256S_SLOT(nq, b) + nf * 2048);       \
        wq[nq][nf][1] = *reinterpret_cast<const frag*>(smem + wb[1] + P256S_SLOT(nq, b) + nf * 2048);       \
    }
#define P256S_MMA16_HALF(mq, nq, s)                                                                          \
    _Pragma("unroll") for (int nf = 0; nf < 2; ++nf)                                                        \
        _Pragma("unroll") for (int mf = 0; mf < 4; ++mf)                                                    \
            acc[(nq) * 2 + nf][(mq) * 4 + mf] = MfmaIn<IN_T>::mma(                                          \
                wq[nq][nf][s], am[mf][s], acc[(nq) * 2 + nf][(mq) * 4 + mf]);
// 16 MFMAs at wave priority 1, 0 outside (other priorities inside / outside the MFMA part: no effect, round 4). The two
// sched_barriers between the halves are where the split-staging experiment issued its piece.
#define P256S_MMA16(mq, nq)                                                                                  \
    {                                                                                                       \
        __builtin_amdgcn_s_setprio(1);                                                                      \
        P256S_MMA16_HALF(mq, nq, 0)                                                                         \
        __builtin_amdgcn_sched_barrier(0);                                                                  \
        __builtin_amdgcn_sched_barrier(0);                                                                  \
        P256S_MMA16_HALF(mq, nq, 1)                                                                         \
        __builtin_amdgcn_s_setprio(0);                                                                      \
    }

// ---- one K-tile out of buffer B: four phases [reads + one slot's staging + wait] B [MFMAs] B. The wait that retires a slot
// sits in the read part of the phase BEFORE the one that reads it (both halves' waits and a barrier precede both halves'
// reads); a slot is restaged in the phase AFTER its last read. P0 / P1 / P3 = post-epilogue form of the three waits; FIN is
// handed to the kernel's phase-3 hook; HALF = a half tile: phases 2 and 3 keep their staging, waits and barriers only.
#define P256S_KTILE(B, P0, P1, P3, FIN, HALF)                                                                \
    {                                                                                                       \
        KT_READ_A(B, 0);                                                                                    \
        KT_READ_W(B, 0);                                                                                    \
        P256S_STAGE(1, (B) ^ 1, oA1 + mA1, oW1, mA1 != 0); /* A m1 of K-tile t+1 */                         \
        p256s_late_reads_done(wm);                                                                          \
        KT_WAIT(P0, B, 0);                /* retires W n1 of this K-tile */                                 \
        p256s_barrier();                                                                                    \
        KT_MMA(0, 0);                                                                                       \
        p256s_barrier();                                                                                    \
        KT_READ_W(B, 1);                                                                                    \
        P256S_STAGE(0, B, oA2, oW2, true);        /* A m0 of K-tile t+2 */                                  \
        p256s_late_reads_done(wm);                                                                          \
        KT_WAIT(P1, B, 1);                /* retires A m1 of this K-tile */                                 \
        p256s_barrier();                                                                                    \
        KT_MMA(0, 1);                                                                                       \
        p256s_barrier();                                                                                    \
        if constexpr (!(HALF)) { KT_READ_A(B, 1); }                                                         \
        P256S_STAGE(2, B, oA2, oW2, true);        /* W n0 of K-tile t+2; nothing new is read in the next phase: no wait */ \
        p256s_late_reads_done(wm);                                                                          \
        p256s_barrier();                                                                                    \
        if constexpr (!(HALF)) { KT_MMA(1, 1); }                                                            \
        p256s_barrier();                                                                                    \
        P256S_STAGE(3, B, oA2, oW2, true);        /* W n1 of K-tile t+2 */                                  \
        KT_PHASE3(FIN);                                                                                     \
        KT_WAIT(P3, B, 3);                /* retires A m0 / W n0 of the next K-tile */                      \
        p256s_barrier();                                                                                    \
        if constexpr (!(HALF)) { KT_MMA(1, 0); }                                                            \
        p256s_barrier();                                                                                    \
        KT_ADVANCE();                                                                                       \
    }
// A K-tile PAIR (buffer 0, buffer 1). Whatever a wave issues between two pairs — an epilogue's stores and pieces, a piece at
// the pair's head — is younger than the slots the pair's first FOUR waits retire (all three of buffer 0, the first of
// buffer 1) and older than what the fifth retires: POST = those four waits allow for it. FIN goes to buffer 0's phase 3.
#define P256S_PAIR(POST, FIN, HALF)                                                                          \
    {                                                                                                       \
        P256S_KTILE(0, POST, POST, POST, FIN, HALF);                                                        \
        P256S_KTILE(1, POST, false, false, false, HALF);                                                    \
    }

// ---- prologue: K-tile 0 completely, K-tile 1 except its A m1 slot (staged by phase 0 of K-tile 0) — the same operations per
// slot and wave as in the loop, in the same order: the counted waits depend on it. Then position t+1 = K-tile 1, t+2 =
// K-tile 2 (KA / KW: bytes of a K-tile in a row of A / W), all but the five youngest slot loads (NWAIT operations) have
// landed — A m0 / W n0 of K-tile 0 and whatever was issued in front of them — and the lower half falls one barrier behind.
#define P256S_PROLOGUE(LIVE1, KA, KW, NWAIT)                                                                 \
    {                                                                                                       \
        char* d0 = smem + stage_dst;                                                                        \
        P256S_STAGE_TO(d0 + P256S_SLOT(0, 0), 0, 0, oA1, oW1, true);                                        \
        P256S_STAGE_TO(d0 + P256S_SLOT(2, 0), 2, 0, oA1, oW1, true);                                        \
        P256S_STAGE_TO(d0 + P256S_SLOT(3, 0), 3, 0, oA1, oW1, true);                                        \
        if (LIVE1) {                                                                                        \
            P256S_STAGE_TO(d0 + P256S_SLOT(1, 0), 1, 0, oA1 + mA1, oW1, true);                              \
        } else { /* (a half tile first: mA1 = 0, written out — gemm256p8_kernel's form of this slot) */     \
            P256S_STAGE_TO(d0 + P256S_SLOT(1, 0), 1, 0, oA1, oW1, false);                                   \
        }                                                                                                   \
        P256S_STAGE_TO(d0 + P256S_SLOT(0, 1), 0, 1, oA2, oW2, true);                                        \
        P256S_STAGE_TO(d0 + P256S_SLOT(2, 1), 2, 1, oA2, oW2, true);                                        \
        P256S_STAGE_TO(d0 + P256S_SLOT(3, 1), 3, 1, oA2, oW2, true);                                        \
        oA1 = oA2; oW1 = oW2;                                                                               \
        oA2 += (KA); oW2 += (KW);                                                                           \
        k2 = 2;                                                                                             \
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NWAIT) : "memory");                                        \
        p256s_barrier();                                                                                    \
        if (wm == 1) p256s_barrier();                                                                       \
    }

// ---- the tile driver of the two tile GEMMs: this workgroup's whole tiles, then its half tile, as one stream. The first pair
// of every tile but the first runs behind an epilogue: POST.
#define P256S_TILE_PAIRS(BEHIND_EPILOGUE, HALF)                                                              \
    for (int kp = 0; kp < npair; ++kp) {                                                                    \
        KT_PAIR_HEAD(kp);                                                                                   \
        if (BEHIND_EPILOGUE) {                                                                              \
            P256S_PAIR(true, false, HALF);                                                                  \
        } else {                                                                                            \
            P256S_PAIR(false, true, HALF);                                                                  \
        }                                                                                                   \
    }
#define P256S_RUN_TILES(TABLE)                                                                               \
    for (int ti = 0; ti < nfull; ++ti) {                                                                    \
        P256S_TILE_PAIRS(kp == 0 && ti > 0, false)                                                          \
        /* The tile is complete. The upper half waits one barrier for the lower half's last MFMAs, both run the epilogue */ \
        /* side by side, then the lower half falls one barrier behind again. */                             \
        if (wm == 0) p256s_barrier();                                                                       \
        epilogue(std::integral_constant<int, 8>{}, 0, ti & 1);                                              \
        KT_AFTER_EPILOGUE();                                                                                \
        if (ti + 1 < mine) {                                                                                \
            p256s_tile_of(smem + (TABLE), ti + 1, cbm, cbn, chalf);                                         \
            stage_x(cbm, cbn, (ti + 1) & 1);                                                                \
            if (wm == 1) p256s_barrier();                                                                   \
        }                                                                                                   \
    }                                                                                                       \
    /* The half tile of the last round, if this workgroup has one (always behind at least one whole tile: POST waits). */ \
    /* Out of the loop above so that the upper accumulators are plainly dead here (inside it the compiler kept them */ \
    /* alive through the half tile's K loop and spilled). */                                                \
    if (nhalf) {                                                                                            \
        P256S_TILE_PAIRS(kp == 0, true)                                                                     \
        if (wm == 0) p256s_barrier();                                                                       \
        epilogue(std::integral_constant<int, 4>{}, chalf == 2 ? 64 : 0, nfull & 1);                         \
    }                                                                                                       \
    /* the unconditional staging of the last K-tiles is still in flight: LDS must not be handed on with DMA writes pending */ \
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
