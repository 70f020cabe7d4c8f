// p256_deal.h — how the persistent 256x256 GEMMs (gemm256p_kernel, gemm256p8_kernel) deal a GEMM's T tiles to their G
// workgroups, and how one dealt tile is packed into a workgroup's tile table. Plain C++, no HIP include: the kernels, their
// launchers and a host-only test program (tests/test_p256_deal_cpu.py) all take the rule from here.
//
// Tiles are dealt in rounds of G: in round i workgroup pb (its position among the workgroups of its XCD first, xcd_remap)
// takes tile i * G + pb of one banded global order (tile_order: bands of 8 row blocks x all column tiles, m fastest inside
// a band: an XCD's 32 tiles of a round are 8 row blocks x 4 column tiles). A LAST round of at most G/2 tiles is dealt in
// HALVES — the m0 rows (wm * 128 + 0..63) and the m1 rows (+64) of a tile go to neighbouring workgroups: FC1 at 12 800 rows
// has 600 tiles = 2 rounds + 88, i.e. 3 tile times for 2.34 tiles of work per CU; as 176 half tiles the tail costs ~0.65 of
// a tile time (a half tile runs phases 0 and 1 of every K-tile with MFMAs and keeps the other two for their staging, waits
// and barriers only).
// (Per-XCD row-block ranges, with A panels meant to stay in the L2 across an XCD's rounds, measured the same time and the
// same fabric reads — FETCH_SIZE x 2 = 120 MB per FC1 launch: one round streams 4.6 MB of distinct operand bytes through
// the XCD's 4 MB L2 — and cannot balance a tail; profiles/gemm_p256_r03.txt.)
#pragma once

#if defined(__HIPCC__)
#define P256_HD __host__ __device__
#else
#define P256_HD
#endif

constexpr int p256_cus = 256;                 // one workgroup per CU
constexpr int p256_table_entries = 64;        // a workgroup's tile table in LDS (256 bytes)
constexpr int p256_max_tiles = 48 * p256_cus; // what the *_ok functions admit
// a workgroup takes one tile of every whole round and at most one (whole or half) tile of the last
static_assert(p256_max_tiles / p256_cus + 1 <= p256_table_entries, "a workgroup's tiles must fit its table");

P256_HD inline int p256_grid(int T) { return T >= p256_cus ? p256_cus : T; }

struct P256Deal {
    int G, pb;
    int full_rounds, rem;
    bool halves;        // the last round is dealt in half tiles
    int nfull, nhalf;   // whole tiles of this workgroup + at most one half tile, always last (and never first: the POST waits
                        // of the half-tile loop assume a whole tile in front of it)
    int mine;           // table entries of this workgroup
    // entry i of the workgroup's table (P256_ENTRY_RULE below): is it a half tile, the m1 half; its index in the global order
    P256_HD bool is_half(int i) const;
    P256_HD bool is_m1_half(int i) const;
    P256_HD int tile(int i) const;
};

// The rule, as declarations of full_rounds, rem, halves, nfull, nhalf and mine in the scope that expands it: p256_deal() below
// for host code, and the kernels directly — through p256_deal() (inlined) the same values came out of the compiler in another
// order, which moved instructions in front of the kernels' K loops.
#define P256_DEAL_RULE(T, G, pb)                                                                             \
    const int full_rounds = (T) / (G), rem = (T) - full_rounds * (G);                                       \
    const bool halves = full_rounds >= 1 && rem > 0 && 2 * rem <= (G);                                      \
    const int nfull = full_rounds + ((!halves && (pb) < rem) ? 1 : 0);                                      \
    const int nhalf = (halves && (pb) < 2 * rem) ? 1 : 0;                                                   \
    const int mine = nfull + nhalf;
// ... and entry i of the table, beside the names of P256_DEAL_RULE: hf = a half tile, L = its index in the global order;
// P256_ENTRY_M1 = that half is the tile's m1 rows
#define P256_ENTRY_RULE(i, G, pb)                                                                            \
    const bool hf = (i) >= nfull;                                                                           \
    const int L = hf ? full_rounds * (G) + ((pb) >> 1) : (i) * (G) + (pb);
#define P256_ENTRY_M1(pb) (hf && ((pb) & 1))

P256_HD inline P256Deal p256_deal(int T, int G, int pb) {
    P256_DEAL_RULE(T, G, pb)
    return P256Deal{G, pb, full_rounds, rem, halves, nfull, nhalf, mine};
}
P256_HD inline bool P256Deal::is_half(int i) const { P256_ENTRY_RULE(i, G, pb) (void)L; return hf; }
P256_HD inline bool P256Deal::is_m1_half(int i) const { P256_ENTRY_RULE(i, G, pb) (void)L; return P256_ENTRY_M1(pb); }
P256_HD inline int P256Deal::tile(int i) const { P256_ENTRY_RULE(i, G, pb) return L; }

// (host: the MXQ extension of the fp8 kernel has no half-tile epilogue)
inline bool p256_last_round_in_halves(int T) { return p256_deal(T, p256_grid(T), 0).halves; }

// table entry: bm | bn << 16 | half tile << 30 | which half << 31 (bm <= 0xffff is the *_ok functions' business)
#define P256_PACK(bm, bn, half, m1_half) \
    ((unsigned)(bm) | ((unsigned)(bn) << 16) | ((half) ? (1u << 30) : 0u) | ((m1_half) ? (1u << 31) : 0u))
P256_HD inline unsigned p256_pack(int bm, int bn, bool half, bool m1_half) { return P256_PACK(bm, bn, half, m1_half); }
struct P256Tile {
    int bm, bn;
    int half;   // 0 whole tile, 1 / 2 = its m0 / m1 rows only
};
P256_HD inline P256Tile p256_unpack(unsigned pk) {
    P256Tile t;
    t.bm = pk & 0xffff;
    t.bn = (pk >> 16) & 0x3fff;
    t.half = (pk >> 30) ? 1 + (int)(pk >> 31) : 0;
    return t;
}
