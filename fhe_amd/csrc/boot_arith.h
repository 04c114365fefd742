// boot_arith.h -- device-only arithmetic that the 32-bit blind rotations at N = 1024 (bootstrap.hip) and at
// N = 2048 (boot_2k.h, boot_n2k_ginx.hip, boot_n2k_lmk.hip) share; include it from .hip files only.  boot.h stays
// the host-visible interface (argument blocks, layouts, launchers).
//
// Residues are 32-bit words mod Q (Mod, from BootTables).  Signed residues (smont_mul, smont_red, ct_bf_s, gs_bf_s):
// the word read as int32, a Montgomery product in (-Q, Q) (more exactly below |a| Q 2^-32 + Q/2), butterflies of two
// adds with no offset and no reduction; one product with oneR = 2^32 mod Q brings a value back to (-Q, Q).  32-bit
// words leave 16 Q of headroom for Q < 2^27, 8 Q for Q < 2^28, 4 Q for Q < 2^29.  The signed inverse transforms
// place those products by a compile-time plan (red_plan.h, included here; lim_s is its LIM) and apply it with
// red_row, gs_bf_s and gs_last_s.  mont_mul is the unsigned lazy product (result below 2 Q).  Also here: the digit
// decomposition for ND retained digits (DecN, decompose_n), the wave-local LDS hand-off (wave_lds_sync), ModSwitch
// in integers (mod_switch), and FHE_FWD_TIGHT, the one A/B knob both sides read.
// The boundary is deliberate: only what both sides read is here.  What bootstrap.hip alone uses (mont_red, mac4,
// ct_bf, gs_bf, fwd_group4, transpose32, Dec / dec_leg / dec_leg2, other_half, kload, brv5, the other knobs) stays
// there.
#pragma once
#include "arith.h"
#include "boot.h"
#include "red_plan.h"

// Forward-transform bounds from the product itself (round 5): a signed Montgomery product is below
// |y| |w| 2^-32 + Q/2 < (Q / 2^32) |y| + Q/2, so a Cooley-Tukey stage takes a bound B to (1 + Q / 2^32) B + Q/2
// rather than B + Q.  From signed digits (B ~ 0): ten stages stay below 6.67 Q for Q < 2^28 (Q / 2^32 < 1/16),
// inside the 8 Q of 32-bit signed words, so FM 2 needs no reduction (the LMKCDEY accumulator bound grows from
// 2.0 Q to 2.2 Q: four digits < 6.67 Q times keys < Q, 26.7 Q^2 2^-32 + Q/2); and for Q < 2^29 (1/8) five
// stages stay below 3.21 Q < 4 Q, so K1w's QM 2 reduces after five stages and after nine (below 0.9 Q each
// time, 3.84 Q before the second) instead of after three, six and nine; for Q < 2^28 eleven stages stay below
// 7.59 Q < 8 Q, so K1w's QM 1 (STD256Q_LMKCDEY) drops its one reduction.  FHE_FWD_TIGHT=0: the round-4 points.
#ifndef FHE_FWD_TIGHT
#define FHE_FWD_TIGHT 1
#endif

namespace fhe_amd {

namespace {

struct Mod {
    uint32_t Q, Q2, qinv;  // qinv = -Q^-1 mod 2^32
    uint32_t qinvp;        // Q^-1 mod 2^32 (signed Montgomery)
    int32_t nQ;            // -Q (signed Montgomery; see fresh_nq)
    uint32_t oneR;         // 2^32 mod Q: smont_mul(x, oneR) = x mod Q in (-Q, Q)
    uint32_t gpR, gmR;     // BootTables::gpR / gmR (fwd_group4)
};
FHE_DEV Mod make_mod(const BootTables& T) {
    return Mod{T.Q, T.Q2, T.qinv, 0u - T.qinv, -(int32_t)T.Q, T.oneR, T.gpR, T.gmR};
}

// a * bR * 2^-32 mod Q, lazily: result < Q (1 + a / 2^32 * ...) < 2Q for a < 4Q, Q < 2^28
FHE_DEV uint32_t mont_mul(uint32_t a, uint32_t bR, const Mod& m) {
    uint64_t t  = (uint64_t)a * bR;
    uint32_t mm = (uint32_t)t * m.qinv;
    return (uint32_t)((t + (uint64_t)mm * m.Q) >> 32);
}
// v_mad_i64_i32 (a * b + c, 32 x 32 -> 64 signed) in plain C, with -Q re-materialised inside each
// loop body (fresh_nq) so that instruction selection sees a sign-extended 32-bit operand (hoisted,
// the compiler widens -Q into a 64-bit constant and the product becomes 5 instructions)
FHE_DEV int64_t mad_i64_i32(int32_t a, int32_t b, int64_t c) {
    return (int64_t)a * b + c;
}
// signed Montgomery (the Q < 2^27 path): a read as int32, bR < Q -> (a b 2^-32 mod Q) in (-Q, Q)
// for any |a| < 2^31: |a bR - mm Q| < 2^31 Q + 2^31 Q
FHE_DEV uint32_t smont_mul(uint32_t a, uint32_t bR, const Mod& m) {
    const int64_t t  = mad_i64_i32((int32_t)a, (int32_t)bR, 0);
    const int32_t mm = (int32_t)((uint32_t)t * m.qinvp);
    return (uint32_t)(mad_i64_i32(mm, m.nQ, t) >> 32);
}
// signed Montgomery reduction of a 64-bit t, |t| < 2^63 - 2^31 Q: t 2^-32 mod Q in (|t| 2^-32 +- Q/2)
FHE_DEV uint32_t smont_red(int64_t t, const Mod& m) {
    const int32_t mm = (int32_t)((uint32_t)t * m.qinvp);
    return (uint32_t)(mad_i64_i32(mm, m.nQ, t) >> 32);
}
// -Q as a value defined inside the current loop body (an empty asm the optimizer cannot hoist)
FHE_DEV Mod fresh_nq(Mod m) {
    asm volatile("" : "+s"(m.nQ));
    return m;
}
// signed Cooley-Tukey: |x|, |y| < B in, < B + Q out, two adds and no offset
FHE_DEV void ct_bf_s(uint32_t& x, uint32_t& y, uint32_t wR, const Mod& m) {
    const uint32_t t = smont_mul(y, wR, m);
    y                = x - t;
    x                = x + t;
}
// signed Gentleman-Sande: x' = x + y, y' = (x - y) w in (-Q, Q); |x| + |y| must stay below 2^31, which the
// reduction plan (red_plan.h) sees to
FHE_DEV void gs_bf_s(uint32_t& x, uint32_t& y, uint32_t wR, const Mod& m) {
    const uint32_t t = x + y;
    y                = smont_mul(x - y, wR, m);
    x                = t;
}
// x w + y z as one unreduced 64-bit chain and one signed Montgomery reduction (a two-term leg): below
// (|x| + |y|) Q 2^-32 + Q/2 in absolute value for w, z < Q
FHE_DEV uint32_t smont_mul2(uint32_t x, uint32_t wR, uint32_t y, uint32_t zR, const Mod& m) {
    return smont_red(mad_i64_i32((int32_t)x, (int32_t)wR, mad_i64_i32((int32_t)y, (int32_t)zR, 0)), m);
}
// Two signed Cooley-Tukey stages as one 4-point group: the stage on register bit hi (twiddle w1 for both pairs),
// then the one on bit lo (w2 for the pair below hi, w3 above) on {a, b, c, d} = registers {r, r|lo, r|hi, r|hi|lo}.
// Two radix-2 stages give a + w1 c +- w2 (b + w1 d) and a - w1 c +- w3 (b - w1 d); with the product twiddles
// w12 = w1 w2 and w13n = -(w1 w3) (nt.h stage_group_consts) the two second-stage terms are two-term legs of b and
// d, and w1 d is never formed: 11 multiplies and 17 instructions instead of 12 and 20.  Inputs below B give
// outputs below B + (B e + Q/2) + (2 B e + Q/2) = (1 + 3 e) B + Q, e = Q 2^-32 (two radix-2 stages:
// (1 + e)^2 B + (1 + e / 2) Q).
FHE_DEV void ct_group4_s(uint32_t& a, uint32_t& b, uint32_t& c, uint32_t& d, uint32_t w1, uint32_t w2, uint32_t w3,
                         uint32_t w12, uint32_t w13n, const Mod& m) {
    const uint32_t t = smont_mul(c, w1, m);
    const uint32_t U = smont_mul2(b, w2, d, w12, m), V = smont_mul2(b, w3, d, w13n, m);
    const uint32_t a1 = a + t, c1 = a - t;
    a = a1 + U;
    b = a1 - U;
    c = c1 + V;
    d = c1 - V;
}
// Two signed Gentleman-Sande stages as one group: the stage on bit lo (wa for the pair (a, b), wb for (c, d)), then
// the one on bit hi (wg for both pairs: its index drops bit lo).  wag = wa wg, wbgn = -(wb wg).  The sums as two
// radix-2 stages form them; the three products in (-Q, Q) when |a| + |b| + |c| + |d| <= 2^31, which the reduction
// plan sees to (red_plan.h red_plan_group_ok).  11 multiplies and 17 instructions instead of 12 and 20.
FHE_DEV void gs_group4_s(uint32_t& a, uint32_t& b, uint32_t& c, uint32_t& d, uint32_t wa, uint32_t wb, uint32_t wg,
                         uint32_t wag, uint32_t wbgn, const Mod& m) {
    const uint32_t s1 = a + b, s2 = c + d, X = a - b, Y = c - d;
    a = s1 + s2;
    c = smont_mul(s1 - s2, wg, m);
    b = smont_mul2(X, wa, Y, wb, m);
    d = smont_mul2(X, wag, Y, wbgn, m);
}
// LIM of the plans: the bound on |x| + |y| (units of Q/10) that keeps sums below 2^31: 16 Q for Q < 2^27,
// 8 Q for Q < 2^28
constexpr int lim_s(bool lz) { return lz ? 160 : 80; }
// the registers a plan row marks (RedPlan::red[s], redT[k]) back to (-Q, Q)
template <int R>
FHE_DEV void red_row(uint32_t (&v)[R], const bool (&row)[R], uint32_t oneR, const Mod& m) {
#pragma unroll
    for (int r = 0; r < R; ++r)
        if (row[r]) v[r] = smont_mul(v[r], oneR, m);
}
// a pair of the last inverse stage (transformnat-impl.h:599-623; the N^-1 factor is already in the data) to
// canonical [0, Q): the sum, |x + y| < 2^fin Q (RedPlan::fin), by adding 2^fin Q and fin + 1 conditional
// subtractions, the product (in (-Q, Q)) by min(d, d + Q) on the unsigned words
FHE_DEV void gs_last_s(uint32_t& x, uint32_t& y, int fin, uint32_t w1R, const Mod& m) {
    uint32_t s = x + y + (m.Q << fin);
#pragma unroll
    for (int f = fin; f >= 0; --f) s = csub(s, m.Q << f);
    const uint32_t d = smont_mul(x - y, w1R, m);
    x                = s;
    y                = min(d, d + m.Q);
}

// intra-wave LDS hand-off: orders this wave's LDS accesses around a layout change
FHE_DEV void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ModSwitch RoundqQ (lwe-pke.cpp:41-46): floor(0.5 + v*to/from) mod to, in IEEE double in
// the reference.  For v*to < 2^53, v < from and odd `from` (or power-of-two from/to) the
// double expression never crosses a rounding boundary, so it equals the exact integer
// floor((2 v to + from) / (2 from)) (proof in DESIGN.md, exhaustively tested).
FHE_DEV uint32_t mod_switch(uint64_t v, uint64_t from, uint64_t to) {
    uint64_t r = (2 * v * to + from) / (2 * from);
    return (uint32_t)(r % to);
}

// SignedDigitDecompose (rgsw-acc.cpp:54-91) for digitsG = ND + 1, as decompose2 with SG: the
// balanced digits 1..ND of the centred value d are the signed bit fields j g of (d + C) ^ M,
// C = 2^(g-1) sum_{j <= ND} 2^(jg), M = 2^(g-1) sum_{1 <= j <= ND} 2^(jg) (needs (ND + 1) g <= 32 and
// C + Q < 2^32; Engine checks both)
struct DecN {
    uint32_t Qh, C, CmQ, g, M;
};
FHE_DEV DecN make_decn(uint32_t Q, uint32_t g, int nd) {
    const uint32_t h = 1u << (g - 1);
    uint32_t C = h, M = 0;
    for (int j = 1; j <= nd; ++j) {
        C += h << (j * g);
        M |= h << (j * g);
    }
    return DecN{Q >> 1, C, C - Q, g, M};
}
template <int ND, int R>
FHE_DEV void decompose_n(uint32_t x, const DecN& c, uint32_t (&d)[ND][R], int r) {
    const uint32_t u = x >= c.Qh ? x + c.CmQ : x + c.C;  // d + C, d = x or x - Q
    const int32_t w  = (int32_t)(u ^ c.M);
#pragma unroll
    for (int j = 0; j < ND; ++j) d[j][r] = (uint32_t)__builtin_amdgcn_sbfe(w, (j + 1) * c.g, c.g);
}

}  // namespace

}  // namespace fhe_amd
