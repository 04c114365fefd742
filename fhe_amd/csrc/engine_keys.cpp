// engine_keys.cpp -- Engine's resident tables and keys: the twiddle / monomial tables of each kernel family, the
// packers from the raw reference layouts into the kernel-native ones, load_bsk / load_ksk, copy_keys_from and
// keygen_device.  See engine.h.
#include <algorithm>
#include <string>

#include "engine.h"
#include "keygen.h"
#include "nt.h"

namespace fhe_amd {

// K1w tables (boot_n2k_ginx.hip k_blind_rotate_n2k): Table / TableI (2048 words each, u32 Montgomery; the
// uniform stages read words 0..31 of them), the half-resolution monomial pairs psi^(2f) - 1 for
// f in [0, 2048] at f + (f >> 5)
void Engine::build_tables_n2k() {
    const uint64_t Q = p_.Q;
    HostNtt h;
    h.init(p_.N, Q, p_.psi);
    constexpr size_t kMono = 2048 + 1 + 64;
    std::vector<uint32_t> t(2048 + 2048 + 2 * kMono, 0);
    uint32_t* tabF = t.data();
    uint32_t* tabI = tabF + 2048;
    uint32_t* mono = tabI + 2048;
    uint32_t* monoP = mono + kMono;
    for (uint32_t i = 0; i < 2048; ++i) {
        tabF[i] = to_mont(h.tab[i], Q);
        tabI[i] = to_mont(h.tabI[i], Q);
    }
    // q = 2N (odd exponents): psi^g - 1 for g in [0, 2048], the kernel negating past 2048 (FULL)
    const uint64_t psi2 = p_.q == 2 * p_.N ? p_.psi : mulmod(p_.psi, p_.psi, Q);
    uint64_t x = 1;
    for (uint32_t f = 0; f <= 2048; ++f) {
        mono[f + (f >> 5)]  = to_mont(submod(x, 1, Q), Q);
        monoP[f + (f >> 5)] = (uint32_t)submod(x, 1, Q);
        x = mulmod(x, psi2, Q);
    }
    FHE_HIP_CHECK(hipSetDevice(device_));
    d_tables2k_.alloc(device_, t.size() * 4);
    FHE_HIP_CHECK(hipMemcpy(d_tables2k_, t.data(), t.size() * 4, hipMemcpyHostToDevice));
    const uint32_t* d = d_tables2k_.as<const uint32_t>();
    tabs2k_ = BootTables{};
    tabs2k_.tabF = d;
    tabs2k_.tabI = d + 2048;
    tabs2k_.twA_fwd = tabs2k_.tabF;
    tabs2k_.twA_inv = tabs2k_.tabI;
    tabs2k_.mono = d + 4096;
    tabs2k_.monoP = tabs2k_.mono + kMono;
    tabs2k_.Q = (uint32_t)Q;
    tabs2k_.Q2 = (uint32_t)(2 * Q);
    tabs2k_.qinv = neg_inv32((uint32_t)Q);
    tabs2k_.ninvR = to_mont(h.ninv, Q);
    tabs2k_.w1R = to_mont(h.tabI[1], Q);
    tabs2k_.oneR = to_mont(1, Q);
    tabs2k_.nR = to_mont(p_.N, Q);
}

// K1w key layout, u32 Montgomery with N^-1 folded in, per index i and wave c:
// [c][q < 6][k2 < 16][64][4] = (K+[r], K+[r+1], K-[r], K-[r+1]), r = 2 k2 + e, slot x(L, r) of layout C,
// q = 2 j + o: digit row 2 j + c, column c (o = 0) or 1 - c (o = 1); raw BSK [n][2][dG2 = 6][2][N]
// LMKCDEY (k_blind_rotate_lmk2k): ek [i][c][q < 6][k4 < 8][64][4], register r = 4 k4 + e4 of lane L is
// slot x(L, r), q = 2 j + o: row 2 j + c, column c (o = 0) or 1 - c (o = 1), from [n][dG2 = 6][2][N];
// then ak [t][q < 6][k4][64][4], q = 2 d + column, from [numAutoKeys + 1][3][2][N]
void Engine::pack_n2k(const uint64_t* bsk) {
    const uint32_t n = p_.n, N = p_.N, dG2 = p_.digitsG2;
    const uint64_t Q = p_.Q, ninv = invmod(N, Q);
    auto word = [&](uint64_t v) { return to_mont(mulmod(v % Q, ninv, Q), Q); };
    auto slot = [](uint32_t L, uint32_t r) { return ((r >> 1) << 7) | (L << 1) | (r & 1); };
    if (p_.method == M_LMKCDEY) {
        const uint32_t nd = p_.digitsG - 1, kq = 2 * nd;  // retained digits, key vectors per slot
        const size_t per = (size_t)2 * kq * 8 * 64 * 4, aper = (size_t)kq * 8 * 64 * 4;
        const size_t nauto = (size_t)p_.numAutoKeys + 1;
        std::vector<uint32_t> dev((size_t)n * per + nauto * aper);
#pragma omp parallel for schedule(static)
        for (int64_t i = 0; i < (int64_t)n; ++i)
            for (uint32_t c = 0; c < 2; ++c)
                for (uint32_t q = 0; q < kq; ++q)
                    for (uint32_t k4 = 0; k4 < 8; ++k4)
                        for (uint32_t L = 0; L < 64; ++L)
                            for (uint32_t e = 0; e < 4; ++e) {
                                const uint32_t row = 2 * (q >> 1) + c, col = (q & 1) ? 1 - c : c;
                                const size_t src = (((size_t)i * dG2 + row) * 2 + col) * N + slot(L, 4 * k4 + e);
                                dev[(size_t)i * per + ((((c * kq + q) * 8 + k4) * 64 + L) * 4 + e)] = word(bsk[src]);
                            }
        const uint64_t* asrc = bsk + (size_t)n * dG2 * 2 * N;
        uint32_t* adst = dev.data() + (size_t)n * per;
        for (size_t t = 0; t < nauto; ++t)
            for (uint32_t q = 0; q < kq; ++q)
                for (uint32_t k4 = 0; k4 < 8; ++k4)
                    for (uint32_t L = 0; L < 64; ++L)
                        for (uint32_t e = 0; e < 4; ++e) {
                            const uint32_t d = q >> 1, col = q & 1;
                            adst[t * aper + (((q * 8 + k4) * 64 + L) * 4 + e)] =
                                word(asrc[((t * nd + d) * 2 + col) * N + slot(L, 4 * k4 + e)]);
                        }
        FHE_HIP_CHECK(hipSetDevice(device_));
        d_bsk2_.alloc(device_, dev.size() * 4);
        FHE_HIP_CHECK(hipMemcpy(d_bsk2_, dev.data(), dev.size() * 4, hipMemcpyHostToDevice));
        return;
    }
    const uint32_t kq = 2 * (p_.digitsG - 1);  // retained digits x 2 columns
    const size_t per = (size_t)2 * kq * 16 * 64 * 4;
    std::vector<uint32_t> dev((size_t)n * per);
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < (int64_t)n; ++i)
        for (uint32_t c = 0; c < 2; ++c)
            for (uint32_t q = 0; q < kq; ++q)
                for (uint32_t k2 = 0; k2 < 16; ++k2)
                    for (uint32_t L = 0; L < 64; ++L)
                        for (uint32_t e4 = 0; e4 < 4; ++e4) {
                            const uint32_t r = 2 * k2 + (e4 & 1), ks = e4 >> 1;
                            const uint32_t x = ((r >> 1) << 7) | (L << 1) | (r & 1);
                            const uint32_t row = 2 * (q >> 1) + c, col = (q & 1) ? 1 - c : c;
                            const size_t src = ((((size_t)i * 2 + ks) * dG2 + row) * 2 + col) * N + x;
                            dev[(size_t)i * per + ((((c * kq + q) * 16 + k2) * 64 + L) * 4 + e4)] =
                                to_mont(mulmod(bsk[src] % Q, ninv, Q), Q);
                        }
    FHE_HIP_CHECK(hipSetDevice(device_));
    d_bsk2_.alloc(device_, dev.size() * 4);
    FHE_HIP_CHECK(hipMemcpy(d_bsk2_, dev.data(), dev.size() * 4, hipMemcpyHostToDevice));
}

// the split kernels' nd = 3 key layouts, u32 Montgomery with N^-1 folded in (as the resident 32-bit
// layouts).  GINX (boot.h g2_key_word) from the raw BSK [n][2][dG2 = 8][2][N]; LMKCDEY
// (launch_blind_rotate_lmk3) from [n][dG2][2][N] ++ [numAutoKeys + 1][3][2][N]
void Engine::pack_ginx3(const uint64_t* bsk) {
    const uint32_t n = p_.n, N = p_.N, dG2 = p_.digitsG2;
    const uint64_t Q = p_.Q, ninv = invmod(N, Q);
    const bool lmk = p_.method == M_LMKCDEY;
    const size_t per = lmk ? 12288 : 8192 * 3, nauto = lmk ? (size_t)p_.numAutoKeys + 1 : 0;
    std::vector<uint32_t> dev((size_t)n * per + nauto * 6144);
    auto word = [&](uint64_t v) { return to_mont(mulmod(v % Q, ninv, Q), Q); };
    if (lmk) {
        // ek [i][c][p < 6][k4 < 4][64][4]: register r = 4 k4 + e of lane L is slot x(L, r)
#pragma omp parallel for schedule(static)
        for (int64_t i = 0; i < (int64_t)n; ++i)
            for (uint32_t c = 0; c < 2; ++c)
                for (uint32_t p = 0; p < 6; ++p)
                    for (uint32_t k4 = 0; k4 < 4; ++k4)
                        for (uint32_t L = 0; L < 64; ++L)
                            for (uint32_t e = 0; e < 4; ++e) {
                                const uint32_t x = (k4 << 8) | (L << 2) | e;
                                const size_t src = (((size_t)i * dG2 + g2_row(c, p, 3)) * 2 + c) * N + x;
                                dev[(size_t)i * per + ((((c * 6 + p) * 4 + k4) * 64 + L) * 4 + e)] = word(bsk[src]);
                            }
        // ak [t][c][d < 3][k4][64][4]
        const uint64_t* asrc = bsk + (size_t)n * dG2 * 2 * N;
        uint32_t* adst = dev.data() + (size_t)n * per;
        for (size_t t = 0; t < nauto; ++t)
            for (uint32_t c = 0; c < 2; ++c)
                for (uint32_t dd = 0; dd < 3; ++dd)
                    for (uint32_t k4 = 0; k4 < 4; ++k4)
                        for (uint32_t L = 0; L < 64; ++L)
                            for (uint32_t e = 0; e < 4; ++e) {
                                const uint32_t x = (k4 << 8) | (L << 2) | e;
                                adst[t * 6144 + ((((c * 3 + dd) * 4 + k4) * 64 + L) * 4 + e)] =
                                    word(asrc[((t * 3 + dd) * 2 + c) * N + x]);
                            }
    } else
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < (int64_t)n; ++i)
        for (uint32_t c = 0; c < 2; ++c)
            for (uint32_t p = 0; p < 6; ++p)
                for (uint32_t k2 = 0; k2 < 8; ++k2)
                    for (uint32_t L = 0; L < 64; ++L)
                        for (uint32_t e4 = 0; e4 < 4; ++e4) {
                            const uint32_t r = 2 * k2 + (e4 & 1), ks = e4 >> 1;
                            const uint32_t x = ((r >> 2) << 8) | (L << 2) | (r & 3);
                            const size_t src = ((((size_t)i * 2 + ks) * dG2 + g2_row(c, p, 3)) * 2 + c) * N + x;
                            dev[(size_t)i * per + g2_key_word(3, c, p, k2, L, e4)] = to_mont(mulmod(bsk[src] % Q, ninv, Q), Q);
                        }
    FHE_HIP_CHECK(hipSetDevice(device_));
    d_bsk2_.alloc(device_, dev.size() * 4);
    FHE_HIP_CHECK(hipMemcpy(d_bsk2_, dev.data(), dev.size() * 4, hipMemcpyHostToDevice));
}

void Engine::build_tables() {
    const uint64_t Q = p_.Q;
    HostNtt h;
    h.init(p_.N, Q, p_.psi);
    constexpr size_t kGroupOff = 32 + 32 + 992 + 992 + 2 * (kMonoHalfWords + kMonoTableWords) + 2048;
    std::vector<uint32_t> t(kGroupOff + 2 * (kGroupUniWords + kGroupLaneWords), 0);
    uint32_t* twAf = t.data();
    uint32_t* twAi = twAf + 32;
    uint32_t* twBf = twAi + 32;
    uint32_t* twBi = twBf + 992;
    uint32_t* mono = twBi + 992;
    uint32_t* monoF = mono + kMonoHalfWords;
    uint32_t* monoP = monoF + kMonoTableWords;
    uint32_t* monoPF = monoP + kMonoHalfWords;
    uint32_t* tabI = monoPF + kMonoTableWords;
    uint32_t* tabF = tabI + 1024;
    for (uint32_t i = 0; i < 1024 && i < p_.N; ++i) {
        tabI[i] = to_mont(h.tabI[i], Q);
        tabF[i] = to_mont(h.tab[i], Q);
    }
    for (int i = 0; i < 32; ++i) {
        twAf[i] = to_mont(h.tab[i], Q);
        twAi[i] = to_mont(h.tabI[i], Q);
    }
    // the signed forward passes read Table[1..3] only through these two constants: no table without them
    uint64_t gp = 0, gm = 0;
    if (!fwd_group_consts(Q, h.tab[1], h.tab[2], h.tab[3], &gp, &gm))
        throw std::invalid_argument("build_tables: Table[3] != Table[1] * Table[2] (or Table[1]^2 != -1) mod Q");
    // the signed inverse pass's last 4-register group (bootstrap.hip dec_leg2) relies on the same relation in TableI
    uint64_t ip = 0, im = 0;
    if (!fwd_group_consts(Q, h.tabI[1], h.tabI[2], h.tabI[3], &ip, &im))
        throw std::invalid_argument("build_tables: TableI[3] != TableI[1] * TableI[2] (or TableI[1]^2 != -1) mod Q");
    // the product twiddles of the grouped stage pairs (BootTables::grp), appended: every other block stays where it was
    if (p_.N == 1024) {
        uint64_t gf[kGroupUniWords + kGroupLaneWords], gi[kGroupUniWords + kGroupLaneWords];
        if (!stage_group_table(Q, h.tab.data(), gf) || !stage_group_table(Q, h.tabI.data(), gi))
            throw std::invalid_argument("build_tables: Table[2k] ^ 2 != Table[k] or Table[2k + 1] != Table[1] * Table[2k] mod Q");
        uint32_t* g = t.data() + kGroupOff;
        for (int i = 0; i < kGroupUniWords; ++i) {
            g[i] = to_mont(gf[i], Q);
            g[kGroupUniWords + i] = to_mont(gi[i], Q);
        }
        for (int i = 0; i < kGroupLaneWords; ++i) {
            g[2 * kGroupUniWords + i] = to_mont(gf[kGroupUniWords + i], Q);
            g[2 * kGroupUniWords + kGroupLaneWords + i] = to_mont(gi[kGroupUniWords + i], Q);
        }
    }
    // lane-major tables of the stages on bits 4..0 (bootstrap.hip, twb_off)
    for (int b = 4; b >= 0; --b) {
        const int per = 1 << (4 - b), off = 32 * (per - 1);
        for (int k = 0; k < per; ++k)
            for (int l = 0; l < 32; ++l) {
                const size_t idx = (size_t)(1 << (9 - b)) + (size_t)l * per + k;
                twBf[off + k * 32 + l] = to_mont(h.tab[idx], Q);
                twBi[off + k * 32 + l] = to_mont(h.tabI[idx], Q);
            }
    }
    // EVAL(X^m - 1) at slot j = omega_j^m - 1 with omega_j = psi^(2 brv(j) + 1) (bootstrap.hip,
    // monomial addressing).  Gates (m = a_i * 2N/q, 2N/q = 2) have even exponents: the
    // half-resolution table psi^(2f) - 1, f in [0, 2N].  BootstrapFunc with ciphertext modulus
    // 2N has any exponent: the full table psi^e - 1, e in [0, 4N].  Entry k at k + (k >> 5).
    {
        const uint64_t psi2 = mulmod(p_.psi, p_.psi, Q);
        uint64_t x = 1;
        for (uint32_t f = 0; f <= 2 * p_.N; ++f) {
            mono[f + (f >> 5)] = to_mont(submod(x, 1, Q), Q);
            monoP[f + (f >> 5)] = (uint32_t)submod(x, 1, Q);
            x = mulmod(x, psi2, Q);
        }
        x = 1;
        for (uint32_t e = 0; e <= 4 * p_.N; ++e) {
            monoF[e + (e >> 5)] = to_mont(submod(x, 1, Q), Q);
            monoPF[e + (e >> 5)] = (uint32_t)submod(x, 1, Q);
            x = mulmod(x, p_.psi, Q);
        }
    }
    if (p_.method == M_LMKCDEY) build_loggen();
    d_tables_.alloc(device_, t.size() * 4);
    FHE_HIP_CHECK(hipMemcpy(d_tables_, t.data(), t.size() * 4, hipMemcpyHostToDevice));
    const uint32_t* d = d_tables_.as<const uint32_t>();
    tabs_.twA_fwd = d;
    tabs_.twA_inv = d + 32;
    tabs_.twB_fwd = d + 64;
    tabs_.twB_inv = d + 64 + 992;
    tabs_.mono = d + 64 + 1984;                     // kMonoHalfWords words
    tabs_.mono_full = tabs_.mono + kMonoHalfWords;  // kMonoTableWords words
    tabs_.monoP = tabs_.mono_full + kMonoTableWords;
    tabs_.monoP_full = tabs_.monoP + kMonoHalfWords;
    tabs_.tabI = tabs_.monoP_full + kMonoTableWords;
    tabs_.tabF = tabs_.tabI + 1024;
    tabs_.Q = (uint32_t)Q;
    tabs_.Q2 = (uint32_t)(2 * Q);
    tabs_.qinv = neg_inv32((uint32_t)Q);
    tabs_.ninvR = to_mont(h.ninv, Q);
    tabs_.w1R = to_mont(h.tabI[1], Q);
    tabs_.oneR = to_mont(1, Q);
    tabs_.nR = to_mont(p_.N, Q);
    tabs_.gpR = to_mont(gp, Q);
    tabs_.gmR = to_mont(gm, Q);
    tabs_.grp = p_.N == 1024 ? (uint32_t)kGroupOff : 0u;
}

// logGen of rgsw-cryptoparameters.cpp:115-127 (k_prep_lmk_w's group positions)
void Engine::build_loggen() {
    if (d_logGen_) return;
    const uint32_t M = 2 * p_.N;
    std::vector<int16_t> lg(M, 0);
    uint32_t gp = 1;
    lg[M - gp] = (int16_t)M;
    for (uint32_t i = 1; i < p_.N / 2; ++i) {
        gp = (gp * 5) % M;
        lg[gp] = (int16_t)i;
        lg[M - gp] = (int16_t)-(int32_t)i;
    }
    d_logGen_.alloc(device_, M * sizeof(int16_t));
    FHE_HIP_CHECK(hipMemcpy(d_logGen_, lg.data(), M * sizeof(int16_t), hipMemcpyHostToDevice));
}

void Engine::build_tables_wide() {
    const uint64_t Q = p_.Q;
    const uint32_t N = p_.N;
    HostNtt h;
    h.init(N, Q, p_.psi);
    std::vector<uint64_t> t(6 * (size_t)N);
    for (uint32_t i = 0; i < N; ++i) {
        t[i] = h.tab[i];
        t[N + i] = shoup64(h.tab[i], Q);
        t[2 * N + i] = h.tabI[i];
        t[3 * N + i] = shoup64(h.tabI[i], Q);
    }
    const uint64_t R = (uint64_t)(((u128)1 << 64) % Q);  // Montgomery 1
    uint64_t x = 1;
    for (uint32_t e = 0; e < 2 * N; ++e) {
        t[4 * N + e] = mulmod(x, R, Q);
        x = mulmod(x, p_.psi, Q);
    }
    // the 32-bit policy's copies (A32): Shoup quotients floor(w 2^32 / Q), psi^e 2^32 mod Q
    const size_t w32 = flags_.narrow ? 6 * (size_t)N : 0;  // tab, tabS, tabI, tabIS (N each), psiM (2N)
    std::vector<uint64_t> t32((w32 + 1) / 2, 0);
    uint32_t* n32 = reinterpret_cast<uint32_t*>(t32.data());
    if (flags_.narrow) {
        auto shoup32 = [&](uint64_t w) { return (uint32_t)(((u128)w << 32) / Q); };
        for (uint32_t i = 0; i < N; ++i) {
            n32[i] = (uint32_t)h.tab[i];
            n32[N + i] = shoup32(h.tab[i]);
            n32[2 * N + i] = (uint32_t)h.tabI[i];
            n32[3 * N + i] = shoup32(h.tabI[i]);
        }
        const uint64_t R32 = (1ull << 32) % Q;
        uint64_t y = 1;
        for (uint32_t e = 0; e < 2 * N; ++e) {
            n32[4 * N + e] = (uint32_t)mulmod(y, R32, Q);
            y = mulmod(y, p_.psi, Q);
        }
        wtabs_.narrow = 1;
        wtabs_.Q32 = (uint32_t)Q;
        wtabs_.qinv32 = neg_inv32((uint32_t)Q);
        wtabs_.ninv32 = (uint32_t)h.ninv;
        wtabs_.ninvS32 = shoup32(h.ninv);
        wtabs_.oneM32 = (uint32_t)R32;
        wtabs_.r2_32 = (uint32_t)mulmod(R32, R32, Q);
    }
    t.insert(t.end(), t32.begin(), t32.end());
    d_wtables_.alloc(device_, t.size() * 8);
    FHE_HIP_CHECK(hipMemcpy(d_wtables_, t.data(), t.size() * 8, hipMemcpyHostToDevice));
    const uint64_t* d = d_wtables_.as<const uint64_t>();
    if (flags_.narrow) {
        const uint32_t* d32 = reinterpret_cast<const uint32_t*>(d + 6 * (size_t)N);
        wtabs_.tab32 = d32;
        wtabs_.tabS32 = d32 + N;
        wtabs_.tabI32 = d32 + 2 * N;
        wtabs_.tabIS32 = d32 + 3 * N;
        wtabs_.psiM32 = d32 + 4 * N;
    }
    wtabs_.tab = d;
    wtabs_.tabS = d + N;
    wtabs_.tabI = d + 2 * N;
    wtabs_.tabIS = d + 3 * N;
    wtabs_.psiM = d + 4 * N;
    wtabs_.Q = Q;
    uint64_t inv = Q;  // Q^-1 mod 2^64 (Newton)
    for (int i = 0; i < 6; ++i) inv *= 2 - Q * inv;
    wtabs_.qinv = 0 - inv;
    wtabs_.ninv = h.ninv;
    wtabs_.ninvS = shoup64(h.ninv, Q);
    wtabs_.oneM = R;
    wtabs_.r2 = mulmod(R, R, Q);
}

void Engine::load_bsk(const uint64_t* bsk, size_t words) {
    if (!bsk) throw std::invalid_argument("bsk is null");
    if (words != p_.bsk_words()) throw std::invalid_argument("bsk has wrong length");
    if (flags_.wide) {  // raw layout [n][2][dG2][2][N], Montgomery form K R mod Q (bootstrap_wide.hip), R = 2^64
                  // (u64 words) or 2^32 (u32 words, flags_.narrow)
        const uint64_t Q = p_.Q;
        const unsigned sh = flags_.narrow ? 32 : 64;
        const size_t wb = flags_.narrow ? 4 : 8;
        std::vector<uint64_t> dev((words * wb + 7) / 8);
        uint32_t* d32 = reinterpret_cast<uint32_t*>(dev.data());
        bool bad = false;
#pragma omp parallel for schedule(static) reduction(|| : bad)
        for (int64_t i = 0; i < (int64_t)words; ++i) {
            bad = bad || bsk[i] >= Q;
            const uint64_t v = (uint64_t)(((u128)(bsk[i] % Q) << sh) % Q);
            if (flags_.narrow) d32[i] = (uint32_t)v;
            else dev[i] = v;
        }
        if (bad) throw std::invalid_argument("bsk coefficient not reduced mod Q");
        FHE_HIP_CHECK(hipSetDevice(device_));
        d_bsk_.alloc(device_, words * wb);
        FHE_HIP_CHECK(hipMemcpy(d_bsk_, dev.data(), words * wb, hipMemcpyHostToDevice));
        if (flags_.g3) pack_ginx3(bsk);
        if (flags_.n2k) pack_n2k(bsk);
        return;
    }
    const uint32_t n = p_.n, N = p_.N, dG2 = p_.digitsG2;
    const uint64_t Q = p_.Q;
    if (dG2 != 4) throw std::invalid_argument("device path expects digitsG = 3");
    // device uint2 blocks [..][d][16][64 lanes]: lane = h*32 + l holds slots l*32 + 2k, +1 of
    // component h -- one 512-byte coalesced load per wave-instruction in the kernels.  With
    // kBskHalfSwap the half-1 lanes of position d hold row d ^ 1 (rows come in pairs).
    //   GINX   raw [n][2][dG2][2][N]                 -> [n][2][dG2][16][64]
    //   LMKCDEY raw [n][dG2][2][N] ++ [nA+1][2][2][N] -> [n][dG2][16][64] ++ [nA+1][2][16][64]
    //   AP     raw [n][baseR][digitsR][dG2][2][N]    -> [n][baseR][digitsR][dG2][16][64]
    const size_t nrgsw = p_.method == M_GINX ? (size_t)n * 2
                         : p_.method == M_AP ? (size_t)n * p_.baseR * p_.digitsR
                                             : (size_t)n;  // RGSW keys of dG2 rows
    const size_t nauto = p_.method == M_LMKCDEY ? (size_t)p_.numAutoKeys + 1 : 0;
    const uint32_t dA = p_.digitsG - 1;
    std::vector<uint32_t> dev(nrgsw * dG2 * 2 * N + nauto * dA * 2 * N);
    // keys carry N^-1 (BootTables::w1R): the kernels' last inverse stage skips the N^-1 multiply
    const uint64_t ninv = invmod(N, Q);
    auto pack = [&](const uint64_t* src_key, uint32_t rows, uint32_t* dst_key) {
        for (uint32_t d = 0; d < rows; ++d)
            for (uint32_t k = 0; k < 16; ++k)
                for (uint32_t lane = 0; lane < 64; ++lane) {
                    const uint32_t h = lane >> 5, l = lane & 31;
                    const uint32_t row = kBskHalfSwap ? d ^ h : d;  // boot.h kBskHalfSwap
                    const size_t src = ((size_t)row * 2 + h) * N + l * 32 + 2 * k;
                    const size_t dst = row_off(d, k, lane, 0);  // boot.h
                    dst_key[dst] = to_mont(mulmod(src_key[src] % Q, ninv, Q), Q);
                    dst_key[dst + 1] = to_mont(mulmod(src_key[src + 1] % Q, ninv, Q), Q);
                }
    };
    if (kGinxU4 && p_.method == M_GINX) {
        // (BSK+, BSK-) of index i interleaved per lane (boot.h ginx_u4_off)
#pragma omp parallel for schedule(static)
        for (int64_t i = 0; i < (int64_t)n; ++i)
            for (uint32_t ks = 0; ks < 2; ++ks) {
                const uint64_t* src_key = bsk + ((size_t)i * 2 + ks) * dG2 * 2 * N;
                uint32_t* dst_key = dev.data() + (size_t)i * 2 * dG2 * 2 * N;
                for (uint32_t d = 0; d < dG2; ++d)
                    for (uint32_t k = 0; k < 16; ++k)
                        for (uint32_t lane = 0; lane < 64; ++lane) {
                            const uint32_t h = lane >> 5, l = lane & 31;
                            const uint32_t row = kBskHalfSwap ? d ^ h : d;
                            const size_t src = ((size_t)row * 2 + h) * N + l * 32 + 2 * k;
                            for (uint32_t e = 0; e < 2; ++e)
                                dst_key[ginx_u4_off(ks, d, k, lane, e)] = to_mont(mulmod(src_key[src + e] % Q, ninv, Q), Q);
                        }
            }
    } else {
#pragma omp parallel for schedule(static)
        for (int64_t i = 0; i < (int64_t)nrgsw; ++i)
            pack(bsk + (size_t)i * dG2 * 2 * N, dG2, dev.data() + (size_t)i * dG2 * 2 * N);
    }
    const uint64_t* asrc = bsk + nrgsw * dG2 * 2 * N;
    uint32_t* adst = dev.data() + nrgsw * dG2 * 2 * N;
    for (size_t t = 0; t < nauto; ++t) pack(asrc + t * dA * 2 * N, dA, adst + t * dA * 2 * N);
    for (size_t i = 0; i < words; ++i)
        if (bsk[i] >= Q) throw std::invalid_argument("bsk coefficient not reduced mod Q");
    FHE_HIP_CHECK(hipSetDevice(device_));
    d_bsk_.alloc(device_, dev.size() * 4);
    FHE_HIP_CHECK(hipMemcpy(d_bsk_, dev.data(), dev.size() * 4, hipMemcpyHostToDevice));
    d_autok_ = d_bsk_.as<uint32_t>() + nrgsw * dG2 * 2 * N;
    repack_ginx2();
}

// the two-wave GINX kernels' key layouts, repacked on the device from the resident one: K1s's
// (k_blind_rotate_ginx2, FHE_HIP_GINX_KERNEL=split) or K1x's (k_blind_rotate_ginx2x, the small-batch default)
void Engine::repack_ginx2() {
    if (p_.method == M_LMKCDEY && !flags_.wide && d_bsk_ && flags_.lmk_pin != 1) {  // K1m's two-digit form
        FHE_HIP_CHECK(hipSetDevice(device_));
        const uint32_t nauto = p_.numAutoKeys + 1;
        if (!d_bsk2_) d_bsk2_.alloc(device_, ((size_t)p_.n * 8192 + (size_t)nauto * 4096) * 4);
        FHE_HIP_CHECK(launch_repack_lmkx(d_bsk_, p_.n, nauto, d_bsk2_, stream_));
        FHE_HIP_CHECK(hipStreamSynchronize(stream_));
        return;
    }
    if (p_.method != M_GINX || flags_.wide || !d_bsk_ || flags_.ginx_pin == 1 || (flags_.ginx_pin == 0 && x_batch_ == 0)) return;
    FHE_HIP_CHECK(hipSetDevice(device_));
    if (!d_bsk2_) d_bsk2_.alloc(device_, (size_t)p_.n * 16384 * 4);
    if (flags_.ginx_pin == 2) FHE_HIP_CHECK(launch_repack_ginx2(d_bsk_, p_.n, d_bsk2_, stream_));
    else FHE_HIP_CHECK(launch_repack_ginx2x(d_bsk_, p_.n, d_bsk2_, stream_));
    FHE_HIP_CHECK(hipStreamSynchronize(stream_));
}

void Engine::load_ksk(const uint64_t* A, size_t nA, const uint64_t* B, size_t nB) {
    if (!A || !B) throw std::invalid_argument("ksk is null");
    const size_t rows = p_.ksk_rows();
    if (nA != p_.ksk_rows_all() * p_.n || nB != p_.ksk_rows_all())
        throw std::invalid_argument(p_.timeopt ? "ksk has wrong length (timeOptimization: the map's three switching keys)"
                                               : "ksk has wrong length");
    if (flags_.wide) {  // u64 A [rows][n] ++ B [rows] as given, per key of the map
        bool bad = false;
#pragma omp parallel for schedule(static) reduction(|| : bad)
        for (int64_t r = 0; r < (int64_t)nA; ++r) bad = bad || A[r] >= p_.qKS;
        for (size_t r = 0; r < nB; ++r) bad = bad || B[r] >= p_.qKS;
        if (bad) throw std::invalid_argument("ksk value not reduced mod qKS");
        FHE_HIP_CHECK(hipSetDevice(device_));
        d_wksk_.alloc(device_, (nA + nB) * 8);
        const size_t one = rows * ((size_t)p_.n + 1);
        for (size_t k = 0; k < p_.ksk_keys(); ++k) {
            FHE_HIP_CHECK(hipMemcpy(d_wksk_ + k * one, A + k * rows * p_.n, rows * p_.n * 8, hipMemcpyHostToDevice));
            FHE_HIP_CHECK(hipMemcpy(d_wksk_ + k * one + rows * p_.n, B + k * rows, rows * 8, hipMemcpyHostToDevice));
        }
        if (flags_.ks32w) {  // u32 rows of launch_keyswitch_w32: A then B at column n, zero-padded
            const size_t W = ksk_width(p_.n);
            std::vector<uint32_t> dev(rows * W, 0);
#pragma omp parallel for schedule(static)
            for (int64_t r = 0; r < (int64_t)rows; ++r) {
                for (uint32_t k = 0; k < p_.n; ++k) dev[(size_t)r * W + k] = (uint32_t)A[(size_t)r * p_.n + k];
                dev[(size_t)r * W + p_.n] = (uint32_t)B[r];
            }
            d_ksk32_.alloc(device_, dev.size() * 4);
            FHE_HIP_CHECK(hipMemcpy(d_ksk32_, dev.data(), dev.size() * 4, hipMemcpyHostToDevice));
            return;
        }
        if (!flags_.ks32) return;
        // flags_.ks32: also the u16 rows of the 32-bit key switch (qKS <= 2^16; ks32_set)
    }
    const size_t W = ksk_width(p_.n);
    std::vector<uint16_t> dev(rows * W, 0);
    bool bad = false;
#pragma omp parallel for schedule(static) reduction(|| : bad)
    for (int64_t r = 0; r < (int64_t)rows; ++r) {
        for (uint32_t k = 0; k < p_.n; ++k) {
            const uint64_t v = A[(size_t)r * p_.n + k];
            bad = bad || v >= p_.qKS;
            dev[(size_t)r * W + k] = (uint16_t)v;
        }
        bad = bad || B[r] >= p_.qKS;
        dev[(size_t)r * W + p_.n] = (uint16_t)B[r];
    }
    if (bad) throw std::invalid_argument("ksk value not reduced mod qKS");
    FHE_HIP_CHECK(hipSetDevice(device_));
    d_ksk_.alloc(device_, dev.size() * 2);
    FHE_HIP_CHECK(hipMemcpy(d_ksk_, dev.data(), dev.size() * 2, hipMemcpyHostToDevice));
}

void Engine::copy_keys_from(const Engine& src) {
    if (src.p_.paramset != p_.paramset || src.p_.method != p_.method)
        throw std::invalid_argument("copy_keys_from: another parameter set");
    // the packed layouts also follow knobs each context read from the environment at creation (word size of
    // the wide keys, which layout d_bsk2_ holds, the key switch's row form): a copy between contexts created
    // under different knobs would hand a kernel buffers of another layout
    const int two_src = src.flags_.ginx_pin == 1 ? 0 : src.flags_.ginx_pin == 2 ? 2 : 3;
    const int two_dst = flags_.ginx_pin == 1 ? 0 : flags_.ginx_pin == 2 ? 2 : 3;
    if (src.flags_.wide != flags_.wide || src.flags_.narrow != flags_.narrow || src.flags_.g3 != flags_.g3 || src.flags_.n2k != flags_.n2k || src.flags_.ks32 != flags_.ks32 ||
        src.flags_.ks32w != flags_.ks32w || (!flags_.wide && p_.method == M_GINX && two_src != two_dst) ||
        (!flags_.wide && p_.method == M_LMKCDEY && (src.flags_.lmk_pin == 1) != (flags_.lmk_pin == 1)))
        throw std::invalid_argument("copy_keys_from: the contexts pack their keys in different layouts "
                                    "(created under different FHE_HIP_* kernel settings)");
    if (!src.ready()) throw std::logic_error("copy_keys_from: the source context has no keys");
    if (src.device_ != device_) {
        int can = 0;
        FHE_HIP_CHECK(hipDeviceCanAccessPeer(&can, device_, src.device_));
        if (can) {
            FHE_HIP_CHECK(hipSetDevice(device_));
            const hipError_t e = hipDeviceEnablePeerAccess(src.device_, 0);
            if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) throw HipError(e, "hipDeviceEnablePeerAccess");
            (void)hipGetLastError();
        }
    }
    // one resident buffer: freed here, then the source's block copied whole (none where the source holds none)
    auto dup = [&](DevBuf& dst, const DevBuf& from) {
        dst.release();
        if (!from.bytes()) return;
        dst.alloc(device_, from.bytes());
        if (src.device_ == device_)
            FHE_HIP_CHECK(hipMemcpyAsync(dst.as<>(), from.as<>(), from.bytes(), hipMemcpyDeviceToDevice, stream_));
        else
            FHE_HIP_CHECK(hipMemcpyPeerAsync(dst.as<>(), device_, from.as<>(), src.device_, from.bytes(), stream_));
    };
    sync_streams();
    const_cast<Engine&>(src).sync_streams();
    dup(d_bsk_, src.d_bsk_);
    d_autok_ = src.d_autok_ ? d_bsk_.as<char>() + (static_cast<const char*>(src.d_autok_) - src.d_bsk_.as<const char>())
                            : nullptr;
    dup(d_bsk2_, src.d_bsk2_);
    dup(d_ksk_, src.d_ksk_);
    dup(d_ksk32_, src.d_ksk32_);
    dup(d_wksk_, src.d_wksk_);
    dup(d_pk_, src.d_pk_);  // the public key, when the source holds one
    FHE_HIP_CHECK(hipStreamSynchronize(stream_));
}

void Engine::keygen_device(const uint64_t* sk, size_t n, uint64_t seed, uint64_t* bsk_out, uint64_t* kskA_out,
                           uint64_t* kskB_out) {
    if (!sk) throw std::invalid_argument("secret key is null");
    if (n != p_.n) throw std::invalid_argument("secret key has wrong length");
    const std::vector<uint64_t> s(sk, sk + n);
    if (flags_.wide) {  // every set outside the fast path (keygen_dev_wide.hip)
        for (uint64_t v : s)
            if (v >= p_.qKS) throw std::invalid_argument("secret key not reduced mod qKS");
        keygen_device_wide(s, seed, bsk_out, kskA_out, kskB_out);
        return;
    }
    const size_t words = p_.bsk_words(), rows = p_.ksk_rows();
    FHE_HIP_CHECK(hipSetDevice(device_));
    d_bsk_.release();
    d_ksk_.release();
    d_autok_ = nullptr;
    DevBuf raw;  // the raw layouts, when the caller asked for them
    uint64_t *rb = nullptr, *ra = nullptr, *rk = nullptr;
    try {
        d_bsk_.alloc(device_, words * 4);
        d_ksk_.alloc(device_, rows * ksk_width(p_.n) * 2);
        const size_t raw_words = (bsk_out ? words : 0) + (kskA_out ? rows * p_.n : 0) + (kskB_out ? rows : 0);
        if (raw_words) raw.alloc(device_, raw_words * 8);
        uint64_t* cur = raw.as<uint64_t>();
        if (bsk_out) { rb = cur; cur += words; }
        if (kskA_out) { ra = cur; cur += rows * p_.n; }
        if (kskB_out) rk = cur;
        keygen_bootstrap_device(p_, s, seed, device_, d_bsk_.as<uint32_t>(), d_ksk_, rb, ra, rk, stream_);
        if (rb) FHE_HIP_CHECK(hipMemcpy(bsk_out, rb, words * 8, hipMemcpyDeviceToHost));
        if (ra) FHE_HIP_CHECK(hipMemcpy(kskA_out, ra, rows * p_.n * 8, hipMemcpyDeviceToHost));
        if (rk) FHE_HIP_CHECK(hipMemcpy(kskB_out, rk, rows * 8, hipMemcpyDeviceToHost));
    } catch (...) {
        d_bsk_.release();
        d_ksk_.release();
        throw;
    }
    const size_t nrgsw = p_.method == M_GINX ? (size_t)p_.n * 2
                         : p_.method == M_AP ? (size_t)p_.n * p_.baseR * p_.digitsR
                                             : (size_t)p_.n;
    d_autok_ = d_bsk_.as<uint32_t>() + nrgsw * p_.digitsG2 * 2 * p_.N;
    repack_ginx2();
}

// The 64-bit path's keys generated in place: one pass of keygen_bootstrap_device_wide per key of the map (one
// without timeOptimization), each into its slice of the resident buffers, then the split kernels' second layout
// repacked on the device.  No host buffer of a key's size exists unless the caller asked for the export; the
// switching key's export is read back from d_wksk_, which holds the raw values.
void Engine::keygen_device_wide(const std::vector<uint64_t>& sk, uint64_t seed, uint64_t* bsk_out, uint64_t* kskA_out,
                                uint64_t* kskB_out) {
    const size_t words = p_.bsk_words(), rows = p_.ksk_rows(), n = p_.n, keys = p_.ksk_keys();
    const size_t wb = flags_.narrow ? 4 : 8, one = rows * (n + 1), W = ksk_width(p_.n);
    sync_streams();  // nothing still reads the keys that are replaced
    FHE_HIP_CHECK(hipSetDevice(device_));
    auto drop = [&] {
        d_bsk_.release();
        d_bsk2_.release();
        d_ksk_.release();
        d_ksk32_.release();
        d_wksk_.release();
        d_autok_ = nullptr;
    };
    drop();
    DevBuf raw;  // the raw bootstrapping key, when the caller asked for it
    try {
        d_bsk_.alloc(device_, words * wb);
        FHE_HIP_CHECK(hipMemsetAsync(d_bsk_, 0, words * wb, stream_));  // AP: the j = 0 slots stay zero
        d_wksk_.alloc(device_, keys * one * 8);
        if (flags_.ks32w) {
            d_ksk32_.alloc(device_, rows * W * 4);
            FHE_HIP_CHECK(hipMemsetAsync(d_ksk32_, 0, rows * W * 4, stream_));
        } else if (flags_.ks32) {
            d_ksk_.alloc(device_, rows * W * 2);
            FHE_HIP_CHECK(hipMemsetAsync(d_ksk_, 0, rows * W * 2, stream_));
        }
        if (bsk_out) {
            raw.alloc(device_, words * 8);
            FHE_HIP_CHECK(hipMemsetAsync(raw.as<>(), 0, words * 8, stream_));
        }
        auto one_key = [&](const Params& pb, uint64_t sb, size_t off, size_t k) {
            KgWideOut o;
            o.bsk = d_bsk_.as<char>() + off * wb;
            o.narrow = flags_.narrow;
            o.wksk = d_wksk_ + k * one;
            o.ksk32 = d_ksk32_;  // ks32 / ks32w sets hold one key (no timeOptimization)
            o.ksk16 = d_ksk_;
            o.raw_bsk = bsk_out ? raw.as<uint64_t>() + off : nullptr;
            keygen_bootstrap_device_wide(pb, sk, sb, device_, o, stream_);
        };
        if (p_.timeopt) {  // the three-key map, seeded per base as the host generator seeds it (keygen.cpp)
            for (uint32_t bg : kSignBases) {
                Params pb = p_.with_base(bg);
                pb.timeopt = false;
                one_key(pb, bg == p_.baseG ? seed : seed ^ ((uint64_t)bg * kRngGamma), p_.bsk_offset(bg), p_.ksk_index(bg));
            }
        } else {
            one_key(p_, seed, 0, 0);
        }
        if (flags_.g3 || flags_.n2k) {
            const KgRepackSizes z = keygen_repack_sizes(p_, flags_.g3);
            const size_t nauto = p_.method == M_LMKCDEY ? (size_t)p_.numAutoKeys + 1 : 0;
            d_bsk2_.alloc(device_, (n * z.per + nauto * z.aper) * 4);
            keygen_repack_device(p_, flags_.g3, flags_.narrow, d_bsk_.as<>(), d_bsk2_.as<uint32_t>(), stream_);
        }
        FHE_HIP_CHECK(hipStreamSynchronize(stream_));
        if (bsk_out) FHE_HIP_CHECK(hipMemcpy(bsk_out, raw.as<>(), words * 8, hipMemcpyDeviceToHost));
        for (size_t k = 0; k < keys; ++k) {
            if (kskA_out)
                FHE_HIP_CHECK(hipMemcpy(kskA_out + k * rows * n, d_wksk_ + k * one, rows * n * 8, hipMemcpyDeviceToHost));
            if (kskB_out)
                FHE_HIP_CHECK(hipMemcpy(kskB_out + k * rows, d_wksk_ + k * one + rows * n, rows * 8, hipMemcpyDeviceToHost));
        }
    } catch (...) {
        drop();
        throw;
    }
}

}  // namespace fhe_amd
