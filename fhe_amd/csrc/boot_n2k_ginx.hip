// boot_n2k_ginx.hip -- K1w GINX: the GINX blind rotation at N = 2048 with the accumulator in registers,
// k_blind_rotate_n2k<ND, ACCIO, QM, FULL>: two waves per gate, kW2Gates gates per workgroup, transforms from
// boot_2k.h.  ND = 2..4 retained digits, Q < 2^29 in the modulus classes QM 0 (Q < 2^27), 2 (Q < 2^29: forward
// transform reduced, centred monomial products) and 3 (Q < 2^27 with QM 2's products), half- or full-resolution
// (FULL, q = 2N) monomial table; n2k_supported lists the combinations that exist.  The first section describes the
// QM 0 form the others derive from; QM 2 / 3 and FULL are described at the kernel.
#include "boot_2k.h"

namespace fhe_amd {

// ===========================================================================
// K1w: GINX at N = 2048 with the accumulator in registers (k_blind_rotate_n2k<ND, ACCIO>), written first for the
// Q < 2^27 rows with even monomial exponents (ciphertext modulus q < 2N): STD256Q (digitsG = 4,
// ND = 3 retained digits), which otherwise run the one-gate-per-workgroup accumulator K5
// (bootstrap_wide.hip) with every butterfly through LDS.  As K1s, wave c of a gate owns RLWE
// component c, here as 32 registers x 64 lanes, through the three layouts (x: 11-bit coefficient
// or EVAL slot index)
//   A: lane = x5..x0, register = x10..x6      (COEF; forward stages on bits 10..6, uniform twiddles)
//   B: lane = (x10..x6) << 1 | x0, register = x5..x1   (stages on bits 5..1, per-lane twiddles)
//   C: lane = x6..x1, register = (x10..x7) << 1 | x0   (EVAL; the stage on bit 0)
// with one LDS tile per wave (word of x: x + 2 (x >> 6): A and B conflict-free, C moved as 8-byte
// pairs).  Per index i (AddToAccCGGI, rgsw-acc-cggi.cpp:102-151): wave c inverse-transforms acc_c
// (signed, its own reduction plan), decomposes it into its ND digits (SignedDigitDecompose,
// rgsw-acc.cpp:54-91; rows 2j + c of the RGSW keys) and forward-transforms them; it then multiplies
// its own digits by the key columns of BOTH components: the sum for its own component stays in its
// registers, the other one is reduced to a word per slot and handed to the partner through this
// wave's tile (8 KiB instead of the ND digit polynomials: four gates per CU fit in LDS), and after
// one barrier each wave adds the partner's word.  acc_c <- acc_c + S+_c (X^a - 1) + S-_c (X^-a - 1)
// exactly as in K1s; only the order of the modular additions differs.
// Keys (Engine::pack_n2k, u32 Montgomery with N^-1 folded in), per index and wave c:
//   [c][q < 2 ND][k2 < 16][64 lanes] uint4 = (K+[r], K+[r + 1], K-[r], K-[r + 1]), r = 2 k2, slot
//   x(L, r) of layout C; q = 2 j + o: digit row 2 j + c, column c (o = 0) or 1 - c (o = 1).
// Bounds (Q < 2^27): digits |d| <= 2^(g-1) grow to < 11 Q + 2^(g-1) in the forward transform;
// |S+-| < ND (11 Q + 2^(g-1)) Q; each reduced sum < 2.6 Q; acc < 5.3 Q after the exchange (the
// inverse plan's BIN).
// ===========================================================================
namespace {
#ifndef FHE_N2K_OPAQUE
#define FHE_N2K_OPAQUE 0
#endif
#ifndef FHE_N2K_KPF
#define FHE_N2K_KPF 1   // key chunks requested ahead of their MAC (0: on use)
#endif
constexpr int kW2Gates = 2;               // gates per workgroup (2 waves each)
constexpr int kW2Mono  = 2048 + 1 + 64;   // (plain, Montgomery) pairs psi^(2f) - 1, f in [0, 2048], entry f + (f >> 5)
constexpr int kW2AccBound = 53;           // |acc| < 5.3 Q between indices (units of Q/10)
constexpr size_t w2_lds() { return (size_t)(2048 + 2048 + 2 * kW2Mono + 2 * kW2Gates * kW2Tile) * 4; }
}  // namespace

// QM 2 (2^27 <= Q < 2^29, STD256 / STD256_3 with q = 2048): the forward transform reduced three times
// (fwd_2k_s), the monomial pairs centred to (-Q/2, Q/2] and the product's low word taken signed, so that
// |acc| < 2.6 Q (own wave: |lo mp.x| 2^-32 < Q/4 per column, |hi mp.y| 2^-32 < 3 ND Q^3 2^-65 < 0.07 Q,
// |acc oneR| 2^-32 < A/8, + Q/2; the partner's share without the acc term) fits the 4 Q plan
// FULL (q = 2N, STD256_4: odd monomial exponents): the table holds psi^g - 1 for g in [0, 2048] and
// psi^(g + 2048) - 1 = -(psi^g - 1) - 2 is formed on the fly, (-x - 2, -y - 2R) with 2R centred (|y'| < Q:
// |acc| < 2.93 Q, bound 30)
// QM 3 (round 5): the centred products of QM 2 for Q < 2^27 (STD256Q_3 / STD256Q_4: q = 2N, 4 digits), with QM 0's
// unreduced forward transform and 16 Q inverse plan: |D| < 11 Q + 2^(g-1), |S+-| < 44 Q^2, so each pair's hi part
// times a monomial half adds < 0.05 Q; own word < Q/2 (lo parts) + 0.09 Q + A/32 + Q/2, the partner's the same
// without A: A < 2.25 Q (bound 25)
template <int ND, int QM, bool FULL>
constexpr int kW2Bound = QM == 3 ? 25 : QM == 2 ? (FULL ? (ND == 4 ? 32 : 30) : 27) : kW2AccBound;
#ifndef FHE_N2K_QM3
#define FHE_N2K_QM3 1  // 4-digit K1w GINX at Q < 2^27 in the QM 3 class (0: QM 2, the round-4 form)
#endif
#ifndef FHE_N2K_ONEWAVE
#define FHE_N2K_ONEWAVE 0  // bit 0 / 1: the 4- / 3-digit K1w GINX forms at one wave per SIMD (512 registers)
#endif
template <int ND, bool ACCIO, int QM = 0, bool FULL = false>
__global__ void __launch_bounds__(128 * kW2Gates,
                                  (((FHE_N2K_ONEWAVE & 1) && ND == 4) || ((FHE_N2K_ONEWAVE & 2) && ND == 3)) ? 1 : 2)
    k_blind_rotate_n2k(GateArgs g, BootTables T, const uint4* __restrict__ keys, const uint16_t* __restrict__ idx,
                       const uint32_t* __restrict__ tvb, uint64_t* __restrict__ ext_a, uint64_t* __restrict__ ext_b,
                       const uint32_t* __restrict__ twAf, const uint32_t* __restrict__ twAi) {
    constexpr int kQ = 2 * ND;  // key vectors per slot pair: ND digit rows x 2 columns
    static_assert(!FULL || QM >= 2, "the full-resolution monomials need the centred (QM 2 / 3) products");
    constexpr int BIN = kW2Bound<ND, QM, FULL>, LIM = QM == 2 ? 40 : 160;
    constexpr int QF = QM == 3 ? 0 : QM;  // the forward transform's reduction class
    constexpr bool CEN = QM >= 2;         // centred monomial pairs and signed lo halves
    extern __shared__ __attribute__((aligned(16))) uint32_t sm[];
    uint32_t* s_tab  = sm;
    uint32_t* s_tabI = sm + 2048;
    uint2* s_mono2   = reinterpret_cast<uint2*>(sm + 4096);
    uint32_t* s_tile = sm + 4096 + 2 * kW2Mono;
    for (int i = threadIdx.x; i < 2048; i += blockDim.x) {
        s_tab[i]  = T.tabF[i];
        s_tabI[i] = T.tabI[i];
    }
    for (int i = threadIdx.x; i < kW2Mono; i += blockDim.x) {
        uint32_t mx = T.monoP[i], my = T.mono[i];
        if (CEN) {  // centred: (-Q/2, Q/2]
            mx = mx > T.Q / 2 ? mx - T.Q : mx;
            my = my > T.Q / 2 ? my - T.Q : my;
        }
        s_mono2[i] = make_uint2(mx, my);
    }

    const int wave = threadIdx.x >> 6, L = threadIdx.x & 63;
    const int c = wave & 1;  // RLWE component of this wave
    const uint32_t gslot = blockIdx.x * kW2Gates + (wave >> 1);
    const bool live = gslot < g.count;
    const uint32_t gate = live ? gslot : g.count - 1;  // spare waves shadow the last gate: every wave meets every barrier
    uint32_t* tile    = s_tile + wave * kW2Tile;
    uint32_t* partner = s_tile + (wave ^ 1) * kW2Tile;
    const Mod m0 = make_mod(T);
    const Mod& m = m0;
    __syncthreads();

    // initial accumulator (BootstrapGateCore, binfhe-base-scheme.cpp:556-575): acc1 = NTT(m), acc0 = 0
    uint32_t acc[32];
    if (ACCIO && !g.acc_tv) {
        const uint64_t* src = g.acc_io + ((size_t)gate * 2 + c) * g.N;
#pragma unroll
        for (int r = 0; r < 32; ++r) acc[r] = csub(mont_mul((uint32_t)src[slot_2k(L, r)], T.ninvR, m), m.Q);
    } else if (c == 1) {
        const uint32_t b = tvb[gate], cm = g.ctmod - 1;
        uint32_t tv[1][32];
#pragma unroll
        for (int r = 0; r < 32; ++r) {
            const uint32_t x = ((uint32_t)r << 6) | (uint32_t)L;
            uint32_t v       = 0;
            if (x % g.factor == 0) {
                const uint32_t bx = (b - x / g.factor) & cm;
                v                 = (bx >= g.lb && bx < g.ub) ? g.lv : g.uv;
            }
            tv[0][r] = v;
        }
        fwd_2k_s<1, QF, true>(tv, tile, L, twAf, s_tab, m);
#pragma unroll
        for (int r = 0; r < 32; ++r) acc[r] = smont_mul(tv[0][r], T.ninvR, m);  // (-Q, Q), N^-1 scaled
    } else {
#pragma unroll
        for (int r = 0; r < 32; ++r) acc[r] = 0;
    }

    const uint16_t* gidx = idx + (size_t)gate * g.n;
    const DecN dec       = make_decn(m.Q, g.gbits, ND);
    // monomial of slot x(L, r): e = m (2 brv11(x) + 1) mod 2N, m = a 2N / ctmod even, in half units
    // f = e / 2 = as (32 brv6(L) + 1) + as 2 brv4(r >> 1) mod 2048 (bit 0 of x adds as 2048 = 0)
    // FULL: e = a (32 brv6(L) + 1) + a 2 brv4(r >> 1) + a 2048 (r & 1) mod 4096
    const uint32_t lmul = 32 * (__builtin_bitreverse32((uint32_t)L) >> 26) + 1;
    const uint4* kc     = keys + (size_t)c * (kQ * 16 * 64) + L;
    uint32_t two_r = 0;
    if (FULL) {
        two_r = 2 * T.oneR;
        two_r = two_r >= T.Q ? two_r - T.Q : two_r;
        two_r = two_r > T.Q / 2 ? two_r - T.Q : two_r;
    }
    // u or -u - (2, 2R) by a mask (0 or ~0): no control flow around the MAC
    auto negp = [&](uint2 u, uint32_t sm) {
        return make_uint2(((u.x ^ sm) - sm) - (2u & sm), ((u.y ^ sm) - sm) - (two_r & sm));
    };
    for (uint32_t i = 0; i < g.n; ++i) {
        const Mod m       = fresh_nq(m0);
        const uint32_t as = __builtin_amdgcn_readfirstlane((uint32_t)gidx[i]) >> (FULL ? 0 : 1);
        const uint4* kb   = kc + (size_t)i * (2 * kQ * 16 * 64);
        // the uniform twiddles re-read per index (hoisted, the 62 of them would sit in VGPRs across the loop)
        const uint32_t* twF = twAf;
        const uint32_t* twI = twAi;
        asm volatile("" : "+s"(twF), "+s"(twI));
#if FHE_N2K_OPAQUE
        // the lane index and this wave's tiles opaque per index: the per-lane LDS bases are re-derived
        // inside the body instead of being kept (spilled) across the loop
        int L_o = L;
        uint32_t *tile_o = tile, *partner_o = partner;
        asm volatile("" : "+v"(L_o), "+v"(tile_o), "+v"(partner_o));
        const int L = L_o;
        uint32_t* const tile    = tile_o;
        uint32_t* const partner = partner_o;
#endif
        constexpr int KB = ND == 4 ? 1 : FHE_N2K_KPF + 1;  // 4 digits: no registers for the key ring
        uint4 kq[KB][kQ];
        __syncthreads();  // the partner has read this wave's tile (previous index)
        uint32_t d[ND][32];
#pragma unroll
        for (int r = 0; r < 32; ++r) d[0][r] = acc[r];
        inv_2k_s<BIN, LIM>(d[0], tile, L, twI, s_tabI, T.w1R, m.oneR, m);
#pragma unroll
        for (int r = 0; r < 32; ++r) decompose_n<ND>(d[0][r], dec, d, r);
        fwd_2k_s<ND, QF, true>(d, tile, L, twF, s_tab, m);
        constexpr uint32_t EM = FULL ? 4095u : 2047u;
        const uint32_t fl = (as * lmul) & EM;
#pragma unroll
        for (int q = 0; q < kQ; ++q) kq[0][q] = kb[(q * 16 + 0) * 64];
#pragma unroll
        for (int k2 = 0; k2 < 16; ++k2) {
            if (KB == 2 && k2 + 1 < 16) {
#pragma unroll
                for (int q = 0; q < kQ; ++q) kq[(k2 + 1) % KB][q] = kb[(q * 16 + k2 + 1) * 64];
            } else if (KB == 1 && k2 > 0) {
#pragma unroll
                for (int q = 0; q < kQ; ++q) kq[0][q] = kb[(q * 16 + k2) * 64];
            }
            asm volatile("" ::: "memory");
            const uint32_t ur = __builtin_amdgcn_readfirstlane(
                (as * 2u * (__builtin_bitreverse32((uint32_t)k2) >> 28)) & EM);
            uint2 mp, mn;
            if (FULL) {
                const uint32_t e0 = (fl + ur) & 4095u, en = (4096u - e0) & 4095u;
                const uint32_t g0 = e0 & 2047u, gn = en & 2047u;
                const uint2 t0 = s_mono2[g0 + (g0 >> 5)], tn = s_mono2[gn + (gn >> 5)];
                mp = negp(t0, 0u - ((e0 >> 11) & 1u));
                mn = negp(tn, 0u - ((en >> 11) & 1u));
            } else {
                const uint32_t f = (fl + ur) & 2047u, fn = 2048u - f;
                mp = s_mono2[f + (f >> 5)];
                mn = s_mono2[fn + (fn >> 5)];
            }
            const uint4* q4 = kq[k2 % KB];
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int r = 2 * k2 + e;
                if (FULL && e == 1) {  // odd a: slot r + 1 is 2048 a further
                    mp = negp(mp, 0u - (as & 1u));
                    mn = negp(mn, 0u - (as & 1u));
                }
#pragma unroll
                for (int o = 0; o < 2; ++o) {  // o = 0: this wave's component, 1: the partner's
                    int64_t S1 = 0, S2 = 0;
#pragma unroll
                    for (int j = 0; j < ND; ++j) {
                        const uint4 kv = q4[2 * j + o];
                        S1 += (int64_t)(int32_t)d[j][r] * (int32_t)(e ? kv.y : kv.x);
                        S2 += (int64_t)(int32_t)d[j][r] * (int32_t)(e ? kv.w : kv.z);
                    }
                    int64_t S;
                    if (CEN) {  // S1 = hi 2^32 + lo with lo signed
                        const int32_t l1 = (int32_t)S1, l2 = (int32_t)S2;
                        const int32_t h1 = (int32_t)((S1 - l1) >> 32), h2 = (int32_t)((S2 - l2) >> 32);
                        S = (int64_t)l1 * (int32_t)mp.x + (int64_t)h1 * (int32_t)mp.y;
                        S += (int64_t)l2 * (int32_t)mn.x + (int64_t)h2 * (int32_t)mn.y;
                    } else {
                        S = (int64_t)((uint64_t)(uint32_t)S1 * mp.x) + (int64_t)(int32_t)(S1 >> 32) * (int32_t)mp.y;
                        S += (int64_t)((uint64_t)(uint32_t)S2 * mn.x) + (int64_t)(int32_t)(S2 >> 32) * (int32_t)mn.y;
                    }
                    if (o == 0) {
                        S += (int64_t)(int32_t)acc[r] * (int32_t)T.oneR;
                        acc[r] = smont_red(S, m);
                    } else {
                        tile[(r << 6) | L] = smont_red(S, m);
                    }
                }
            }
        }
        __syncthreads();  // both waves' partner words are in LDS
#pragma unroll
        for (int r = 0; r < 32; ++r) acc[r] += partner[(r << 6) | L];
    }

    if (ACCIO) {  // every wave of the workgroup leaves here: no barrier is skipped by some only
        if (live) {
            uint64_t* dst = g.acc_io + ((size_t)gate * 2 + c) * g.N;
#pragma unroll
            for (int r = 0; r < 32; ++r) {
                const int32_t v = (int32_t)smont_mul(acc[r], T.nR, m);
                dst[slot_2k(L, r)] = (uint64_t)(uint32_t)(v < 0 ? v + (int32_t)m.Q : v);
            }
        }
        return;
    }
    // extraction (binfhe-base-scheme.cpp:110-121): canonical COEF in layout A; wave 0 writes the
    // transposed acc0 (coefficient k -> position N - k, negated), wave 1 the b term from acc1[0]
    __syncthreads();  // the partner has read this wave's tile
    inv_2k_s<BIN, LIM>(acc, tile, L, twAi, s_tabI, T.w1R, m.oneR, m);
    if (!live) return;
    if (c == 0) {
        uint64_t* oa = ext_a + (size_t)gate * g.N;
#pragma unroll
        for (int r = 0; r < 32; ++r) {
            const uint32_t x = ((uint32_t)r << 6) | (uint32_t)L;
            const uint32_t v = acc[r];
            const uint32_t o = (x == 0 || v == 0) ? v : m.Q - v;
            oa[(g.N - x) & (g.N - 1)] = g.msb_out ? mod_switch(o, m.Q, g.qKS) : o;
        }
    } else if (L == 0) {
        const uint32_t bb = add_mod(g.b_const, acc[0], m.Q);
        ext_b[gate]       = g.msb_out ? mod_switch(bb, m.Q, g.qKS) : bb;
    }
}

bool n2k_supported(const GateArgs& g, const BootTables& t, int nd) {
    // The monomial table is full-resolution (psi^g - 1, the kernel negating past psi^2048) exactly when the set's
    // q = 2N, half-resolution (psi^(2f) - 1) otherwise (Engine::build_tables_n2k).  The full-resolution
    // instantiations (3 retained digits at 2^27 <= Q < 2^29, 4 digits) take any ciphertext modulus <= 2N; the
    // half-resolution ones need even exponents, ciphertext moduli below 2N (a seam call at 2N stays on K5).
    // 3 retained digits at Q < 2^29 (Q >= 2^27: QM 2), 2 retained digits at 2^27 <= Q < 2^29.
    const bool full = g.q == 2 * g.N;
    const bool qok = full ? (nd == 4 || (nd == 3 && t.Q >= (1u << 27))) : g.ctmod < 2 * g.N;
    const bool ndok = nd == 3 || (nd == 2 && t.Q >= (1u << 27)) || (nd == 4 && full);
    return t.Q < (1u << 29) && ndok && g.N == 2048 && qok && g.ctmod <= 2 * g.N &&
           g.tv == nullptr && g.tv64 == nullptr && g.gbits >= 2 && (uint32_t)(nd + 1) * g.gbits <= 32;
}

hipError_t launch_blind_rotate_n2k(const GateArgs& g, const BootTables& t, const void* keys, const uint16_t* idx,
                                   const uint32_t* tvb, uint64_t* ext_a, uint64_t* ext_b, int nd, hipStream_t s) {
    if (g.count == 0) return hipSuccess;
    if (!n2k_supported(g, t, nd)) return hipErrorInvalidValue;
    static const bool attr = [] {
        for (const void* k : {reinterpret_cast<const void*>(&k_blind_rotate_n2k<3, false>),
                              reinterpret_cast<const void*>(&k_blind_rotate_n2k<3, true>),
                              reinterpret_cast<const void*>(&k_blind_rotate_n2k<3, false, 2>),
                              reinterpret_cast<const void*>(&k_blind_rotate_n2k<3, true, 2>),
                              reinterpret_cast<const void*>(&k_blind_rotate_n2k<2, false, 2>),
                              reinterpret_cast<const void*>(&k_blind_rotate_n2k<2, true, 2>),
                              reinterpret_cast<const void*>(&k_blind_rotate_n2k<3, false, 2, true>),
                              reinterpret_cast<const void*>(&k_blind_rotate_n2k<3, true, 2, true>),
                              reinterpret_cast<const void*>(&k_blind_rotate_n2k<4, false, 2, true>),
                              reinterpret_cast<const void*>(&k_blind_rotate_n2k<4, true, 2, true>),
                              reinterpret_cast<const void*>(&k_blind_rotate_n2k<4, false, 3, true>),
                              reinterpret_cast<const void*>(&k_blind_rotate_n2k<4, true, 3, true>)})
            (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)w2_lds());
        return true;
    }();
    (void)attr;
    const uint32_t blocks = (g.count + kW2Gates - 1) / kW2Gates;
    const uint4* k = static_cast<const uint4*>(keys);
#define FHE_N2K(ND_, IO, QM_, ...)                                                                                 \
    hipLaunchKernelGGL((k_blind_rotate_n2k<ND_, IO, QM_, ##__VA_ARGS__>), dim3(blocks), dim3(128 * kW2Gates), w2_lds(), \
                       s, g, t, k, idx, tvb, ext_a, ext_b, t.twA_fwd, t.twA_inv)
    if (g.q == 2 * g.N) {  // full-resolution table: STD256_4 (29-bit Q, q = 2N); STD256Q_3 / STD256Q_4 (4 digits)
        if (nd == 4 && FHE_N2K_QM3 && t.Q < (1u << 27)) {  // STD256Q_3 / STD256Q_4: no forward reductions (QM 3)
            if (g.acc_io) FHE_N2K(4, true, 3, true); else FHE_N2K(4, false, 3, true);
        } else if (nd == 4) { if (g.acc_io) FHE_N2K(4, true, 2, true); else FHE_N2K(4, false, 2, true); }
        else if (g.acc_io) FHE_N2K(3, true, 2, true); else FHE_N2K(3, false, 2, true);
    } else if (t.Q < (1u << 27)) {  // STD256Q
        if (g.acc_io) FHE_N2K(3, true, 0); else FHE_N2K(3, false, 0);
    } else if (nd == 3) {  // STD256_3 (29-bit Q)
        if (g.acc_io) FHE_N2K(3, true, 2); else FHE_N2K(3, false, 2);
    } else {  // STD256 (29-bit Q, digitsG 3)
        if (g.acc_io) FHE_N2K(2, true, 2); else FHE_N2K(2, false, 2);
    }
#undef FHE_N2K
    return hipGetLastError();
}

}  // namespace fhe_amd
