// boot_2k.h -- the N = 2048 transforms of the two K1w kernels (boot_n2k_ginx.hip k_blind_rotate_n2k,
// boot_n2k_lmk.hip k_blind_rotate_lmk2k); device only.
//
// Wave c of a gate owns RLWE component c as 32 registers x 64 lanes, through three layouts (x: 11-bit
// coefficient or EVAL slot index):
//   A: lane = x5..x0, register = x10..x6               (COEF; stages on bits 10..6, uniform twiddles twA)
//   B: lane = (x10..x6) << 1 | x0, register = x5..x1   (stages on bits 5..1, per-lane twiddles from LDS)
//   C: lane = x6..x1, register = (x10..x7) << 1 | x0   (EVAL; the stage on bit 0; slot_2k)
// with one LDS tile of kW2Tile words per wave, word of x at x + 2 (x >> 6) (wa2k / wb2k / wc2k: per-lane bases,
// so that every access is base + immediate; A and B conflict-free, C moved as 8-byte pairs).
//   fwd_2k_s<NP, QM>   signed forward transform A -> C of NP polynomials through the one tile; QM is the modulus
//                      class that places its reductions (none for Q < 2^27; see red_2k and FHE_FWD_TIGHT)
//   inv_2k_s<BIN, LIM> signed inverse C -> A from |v| < BIN Q / 10 to canonical [0, Q), with the compile-time
//                      reduction plan of red_plan.h (N2kShape, thresholds searched) for LIM / 10 Q of signed
//                      headroom; the keys carry N^-1, so the last stage scales by TableI[1] (w1R) only
#pragma once
#include "boot_arith.h"

namespace fhe_amd {

namespace {

constexpr int kW2Tile  = 2048 + 64;       // words of one wave's tile
// LDS word of x: x + 2 (x >> 6) (wa2k / wb2k / wc2k below)
// layout C: the EVAL slot of lane L, register r
FHE_DEV uint32_t slot_2k(int L, int r) {
    return ((uint32_t)(r >> 1) << 7) | ((uint32_t)L << 1) | (uint32_t)(r & 1);
}

// signed forward NTT, layout A (|v| < B) -> C (|v| < B + 11 Q), NP polynomials through one tile
// (transposed one after the other); twA: Table[0..31] (uniform), s_tab: Table[0..2047] in LDS
// word of x in each layout as a per-lane base plus a per-register constant (so that every LDS access
// is base + immediate): A x = (r << 6) | L -> L + 66 r; B x = (G << 6) | (r << 1) | j -> 66 G + j + 2 r;
// C pair x = (rh << 7) | (L << 1) -> 2 L + 2 (L >> 5) + 132 rh
FHE_DEV int wa2k(int L) { return L; }
FHE_DEV int wb2k(int L) { return 66 * (L >> 1) + (L & 1); }
FHE_DEV int wc2k(int L) { return 2 * L + 2 * (L >> 5); }

// QM, the modulus class: 0: Q < 2^27 (16Q of signed headroom), no reduction; 1: Q < 2^28 (8Q): one signed
// Montgomery product by 2^32 mod Q after the five A stages (|v| < 5Q + 2^(g-1) -> < 0.82 Q), the six
// stages after it end below 6.82 Q; 2: Q < 2^29 (4Q): one after stages 3, 6 and 9 (< 3Q + 2^(g-1) ->
// < 0.875 Q, < 3.875 Q -> < 0.98 Q, < 3.98 Q -> < Q), the last two end below 3 Q
template <int NP>
FHE_DEV void red_2k(uint32_t (&v)[NP][32], const Mod& m) {
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int r = 0; r < 32; ++r) v[p][r] = smont_mul(v[p][r], m.oneR, m);
}

// one radix-2 stage over the 32 registers: A stages (b = 10..6) pair register bits b - 6 with the twiddles
// of twA; B stages (b = 5..1) pair register bits b - 1 with s_tab's, indexed by the lane pair G
template <int NP, bool B>
FHE_DEV void fwd_2k_stage(uint32_t (&v)[NP][32], int b, int G, const uint32_t* __restrict__ tw, const Mod& m) {
    const int rb = B ? b - 1 : b - 6;
#pragma unroll
    for (int r = 0; r < 32; ++r) {
        if (r & (1 << rb)) continue;
        const uint32_t w = B ? tw[(1 << (10 - b)) + (G << (5 - b)) + (r >> b)] : tw[(1 << (10 - b)) + (r >> (rb + 1))];
#pragma unroll
        for (int p = 0; p < NP; ++p) ct_bf_s(v[p][r], v[p][r | (1 << rb)], w, m);
    }
}

// v - rint(v / Q) Q in 32-bit registers (|v| < 2^31): the float quotient is off by under 2^-20, so the
// result is below 0.51 Q; no 64-bit temporaries (FRED: K1w GINX, whose 3-digit form spilled 104 VGPRs with
// smont_mul's and 30 with this; K1w-LMKCDEY keeps red_2k, measured 6% faster there)
template <int NP>
FHE_DEV void red_2k_f(uint32_t (&v)[NP][32], const Mod& m) {
    const float iq = 1.0f / (float)m.Q;
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int r = 0; r < 32; ++r) {
            const int32_t x = (int32_t)v[p][r];
            const int32_t q = (int32_t)__builtin_rintf((float)x * iq);
            v[p][r]         = (uint32_t)(x - q * (int32_t)m.Q);
        }
}

template <int NP, int QM = 0, bool FRED = false>
FHE_DEV void fwd_2k_s(uint32_t (&v)[NP][32], uint32_t* t, int L, const uint32_t* __restrict__ twA,
                      const uint32_t* s_tab, const Mod& m) {
    // the stages are written out: a loop over them with the reductions inside was left rolled for NP = 3,
    // and a plain one for NP = 4 (the digit array in scratch)
    const int G = L >> 1;
    uint32_t* ta = t + wa2k(L);
    uint32_t* tb = t + wb2k(L);
    uint32_t* tc = t + wc2k(L);
    fwd_2k_stage<NP, false>(v, 10, G, twA, m);
    fwd_2k_stage<NP, false>(v, 9, G, twA, m);
    fwd_2k_stage<NP, false>(v, 8, G, twA, m);
    if (QM == 2 && !FHE_FWD_TIGHT) FRED ? red_2k_f<NP>(v, m) : red_2k<NP>(v, m);  // after stage 3
    fwd_2k_stage<NP, false>(v, 7, G, twA, m);
    fwd_2k_stage<NP, false>(v, 6, G, twA, m);
    if (QM == 1 && !FHE_FWD_TIGHT) red_2k<NP>(v, m);
    if (QM == 2 && FHE_FWD_TIGHT) FRED ? red_2k_f<NP>(v, m) : red_2k<NP>(v, m);  // after stage 5
#pragma unroll
    for (int p = 0; p < NP; ++p) {  // A -> B
#pragma unroll
        for (int r = 0; r < 32; ++r) ta[66 * r] = v[p][r];
        wave_lds_sync();
#pragma unroll
        for (int r = 0; r < 32; ++r) v[p][r] = tb[2 * r];
        wave_lds_sync();
    }
    fwd_2k_stage<NP, true>(v, 5, G, s_tab, m);
    if (QM == 2 && !FHE_FWD_TIGHT) FRED ? red_2k_f<NP>(v, m) : red_2k<NP>(v, m);  // after stage 6
    fwd_2k_stage<NP, true>(v, 4, G, s_tab, m);
    fwd_2k_stage<NP, true>(v, 3, G, s_tab, m);
    fwd_2k_stage<NP, true>(v, 2, G, s_tab, m);
    if (QM == 2) FRED ? red_2k_f<NP>(v, m) : red_2k<NP>(v, m);  // after stage 9
    fwd_2k_stage<NP, true>(v, 1, G, s_tab, m);
#pragma unroll
    for (int p = 0; p < NP; ++p) {  // B -> C
#pragma unroll
        for (int r = 0; r < 32; ++r) tb[2 * r] = v[p][r];
        wave_lds_sync();
#pragma unroll
        for (int rh = 0; rh < 16; ++rh) {
            const uint2 q = *reinterpret_cast<const uint2*>(tc + 132 * rh);
            v[p][2 * rh]     = q.x;
            v[p][2 * rh + 1] = q.y;
        }
        wave_lds_sync();
    }
#pragma unroll
    for (int rh = 0; rh < 16; ++rh) {
        const uint32_t w = s_tab[1024 + (rh << 6) + L];
#pragma unroll
        for (int p = 0; p < NP; ++p) ct_bf_s(v[p][2 * rh], v[p][2 * rh + 1], w, m);
    }
}

// signed inverse NTT, layout C (EVAL, |v| < BIN Q / 10) -> A (COEF), canonical [0, Q); the keys carry
// N^-1, so the last stage scales by TableI[1] only (w1R)
// LIM: the signed headroom in units of Q/10 (160: Q < 2^27; 80: Q < 2^28, where the last stage's
// x + y + (Q << fin) stays below 16 Q < 2^32)
template <int BIN, int LIM = 160>
FHE_DEV void inv_2k_s(uint32_t (&v)[32], uint32_t* t, int L, const uint32_t* __restrict__ twAi,
                      const uint32_t* s_tabI, uint32_t w1R, uint32_t oneR, const Mod& m) {
    constexpr RedPlan<N2kShape> P = red_plan_search<N2kShape>(BIN, LIM);
    const int G = L >> 1;
    uint32_t* ta = t + wa2k(L);
    uint32_t* tb = t + wb2k(L);
    uint32_t* tc = t + wc2k(L);
    red_row(v, P.red[0], oneR, m);
#pragma unroll
    for (int rh = 0; rh < 16; ++rh) gs_bf_s(v[2 * rh], v[2 * rh + 1], s_tabI[1024 + (rh << 6) + L], m);
    // C -> B
    red_row(v, P.redT[0], oneR, m);
#pragma unroll
    for (int rh = 0; rh < 16; ++rh)
        *reinterpret_cast<uint2*>(tc + 132 * rh) = make_uint2(v[2 * rh], v[2 * rh + 1]);
    wave_lds_sync();
#pragma unroll
    for (int r = 0; r < 32; ++r) v[r] = tb[2 * r];
    wave_lds_sync();
#pragma unroll
    for (int b = 1; b <= 5; ++b) {
        const int rb = b - 1;
        red_row(v, P.red[b], oneR, m);
#pragma unroll
        for (int r = 0; r < 32; ++r) {
            if (r & (1 << rb)) continue;
            gs_bf_s(v[r], v[r | (1 << rb)], s_tabI[(1 << (10 - b)) + (G << (5 - b)) + (r >> b)], m);
        }
    }
    // B -> A
    red_row(v, P.redT[1], oneR, m);
#pragma unroll
    for (int r = 0; r < 32; ++r) tb[2 * r] = v[r];
    wave_lds_sync();
#pragma unroll
    for (int r = 0; r < 32; ++r) v[r] = ta[66 * r];
    wave_lds_sync();
#pragma unroll
    for (int b = 6; b <= 9; ++b) {
        const int rb = b - 6;
        red_row(v, P.red[b], oneR, m);
#pragma unroll
        for (int r = 0; r < 32; ++r) {
            if (r & (1 << rb)) continue;
            gs_bf_s(v[r], v[r | (1 << rb)], twAi[(1 << (10 - b)) + (r >> (rb + 1))], m);
        }
    }
    // bit 10, canonical results (gs_last_s)
    red_row(v, P.red[10], oneR, m);
#pragma unroll
    for (int r = 0; r < 16; ++r) gs_last_s(v[r], v[r | 16], P.fin[r], w1R, m);
}

}  // namespace

}  // namespace fhe_amd
