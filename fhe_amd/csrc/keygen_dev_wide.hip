// keygen_dev_wide.hip -- device BTKeyGen for every parameter set outside the N = 1024, digitsG = 3, Q < 2^31 fast
// path of keygen_dev.hip: any N the batched NTT takes (512 / 1024 / 2048 here), Q up to 2^62, any digitsG, any
// qKS / baseKS / n, all three methods, one key of the timeOptimization map per call.
//
// The header of keygen_dev.hip stays the definition: per RGSW row pair A uniform mod Q (drawn in EVALUATION), e the
// table Gaussian with the message monomial folded in (row 1) or kept as M (row 0), forward NTTs of [E, M]
// (ntt_launch on a plan for (Q, psi, N)), then row1 = A S + NTT(e) (- skAuto g), row0 = A + NTT(M).  Bit-identical
// to keygen_bootstrap() (keygen.cpp) for the same (sk, seed); descriptors from keygen_desc.cpp.
//
// Modular products: Q has up to 54 bits here (62 at most), so a product of two residues needs 128 bits.  The finish
// kernel uses Montgomery's REDC with R = 2^64 on the exact product (mul.lo + __umul64hi): mont(a, b) = a b R^-1 mod Q
// for a < Q.  The host hands over S R and skAuto R, so mont(A, S R) = A S exactly; the resident word x R of the
// 64-bit accumulator (bootstrap_wide.hip, load_bsk's wide branch) is mont(x, R^2).  The 32-bit policy's word
// x 2^32 mod Q (Q < 2^30) is one u64 shift and remainder.
//
// Resident layouts written here: d_bsk_ in the raw order [..][dG2][2][N] as x R (u64, R = 2^64) or x 2^32 (u32,
// narrow), no N^-1; d_wksk_ u64 A [rows][n] ++ B [rows]; the u32 / u16 padded rows of the 32-bit key switches.
// The split kernels' second layouts (g3 / n2k) are repacked from the resident d_bsk_ by k_kg_repack, one thread per
// destination word: to_mont(x N^-1) is the resident word times one constant mod Q.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdexcept>
#include <vector>

#include "engine.h"
#include "keygen.h"
#include "keygen_desc.h"
#include "nt.h"
#include "ntt.h"
#include "rng_dev.h"

namespace fhe_amd {
namespace {

// a b R^-1 mod Q, R = 2^64, for a < Q < 2^62 and any b: T = a b < Q R, m = T qneg mod R (qneg = -Q^-1 mod R),
// (T + m Q) / R < 2 Q; the low words cancel, their carry is 1 unless T's low word is 0
__device__ __forceinline__ uint64_t mont_mul(uint64_t a, uint64_t b, uint64_t Q, uint64_t qneg) {
    const uint64_t lo = a * b, hi = __umul64hi(a, b);
    const uint64_t m = lo * qneg;
    const uint64_t t = hi + __umul64hi(m, Q) + (lo != 0);
    return t >= Q ? t - Q : t;
}

__global__ void __launch_bounds__(256) k_kgw_sample(const KgRow* __restrict__ D, uint32_t N, uint64_t Q,
                                                    uint64_t* __restrict__ A, uint64_t* __restrict__ T, DggTable dg) {
    const KgRow k = D[blockIdx.x];
    uint64_t* a = A + (size_t)blockIdx.x * N;
    uint64_t* e = T + (size_t)blockIdx.x * 2 * N;
    uint64_t* m = e + N;
    for (uint32_t j = threadIdx.x; j < N; j += blockDim.x) {
        a[j] = draw_uniform(k.s0, k.call + j, Q);
        uint64_t ev = draw_dgg(k.s0, k.call + N + j, Q, dg);
        uint64_t mv = (k.mval && j == k.mm) ? k.mval : 0;
        if (k.odd) {
            ev += mv;
            ev = ev >= Q ? ev - Q : ev;
            mv = 0;
        }
        e[j] = ev;
        m[j] = mv;
    }
}

struct KgFinish {
    uint64_t Q, qneg, r2;   // -Q^-1 mod 2^64, 2^128 mod Q
    const uint64_t* SR;     // S R mod Q [N]
    const uint64_t* autoR;  // skAuto R mod Q [numAutoKeys + 1][N]
    void* bsk;              // this key's resident words
    uint64_t* raw;          // this key's raw export (or null)
    uint32_t N, narrow;
};

__global__ void __launch_bounds__(256) k_kgw_finish(const KgRow* __restrict__ D, const uint64_t* __restrict__ A,
                                                    const uint64_t* __restrict__ T, KgFinish f) {
    const KgRow k = D[blockIdx.x];
    const uint32_t N = f.N;
    const uint64_t Q = f.Q;
    const uint64_t* a = A + (size_t)blockIdx.x * N;
    const uint64_t* e = T + (size_t)blockIdx.x * 2 * N;
    const uint64_t* m = e + N;
    const size_t base = (size_t)k.rp * 2 * N;
    for (uint32_t j = threadIdx.x; j < N; j += blockDim.x) {
        const uint64_t av = a[j];
        uint64_t r1 = mont_mul(av, f.SR[j], Q, f.qneg) + e[j];
        r1 = r1 >= Q ? r1 - Q : r1;
        if (k.aidx >= 0) {
            const uint64_t t = mont_mul(k.g, f.autoR[(size_t)k.aidx * N + j], Q, f.qneg);
            r1 = r1 >= t ? r1 - t : r1 + Q - t;
        }
        uint64_t r0 = av + m[j];
        r0 = r0 >= Q ? r0 - Q : r0;
        if (f.narrow) {
            uint32_t* b = static_cast<uint32_t*>(f.bsk);
            b[base + j] = (uint32_t)((r0 << 32) % Q);
            b[base + N + j] = (uint32_t)((r1 << 32) % Q);
        } else {
            uint64_t* b = static_cast<uint64_t*>(f.bsk);
            b[base + j] = mont_mul(r0, f.r2, Q, f.qneg);
            b[base + N + j] = mont_mul(r1, f.r2, Q, f.qneg);
        }
        if (f.raw) {
            f.raw[base + j] = r0;
            f.raw[base + N + j] = r1;
        }
    }
}

// One wave per KSK row [N][baseKS][digitsKS]: n uniform draws, <a, s> by wave reduction, b = e + <a, s> + s'_i j B^k.
// <a, s> is exact mod qKS in every regime:
//   * qKS a power of two (up to 2^35 here, n up to 1625): products and sums wrap mod 2^64, which is exact mod 2^k;
//     the same holds for s'_i (j B^k mod qKS);
//   * any other qKS (the primes of TOY / SIGNED_MOD_TEST) must be below 2^32 (checked on the host): a product of two
//     residues fits 64 bits and is reduced at once, so a lane's sum of at most 2048 / 64 terms stays below 2^37 and
//     the wave's below 2^43;
//   * a baseKS that is no power of two (25, 21) only enters through j B^k mod qKS, B^k < qKS taken from the host.
// Every resident form is written in the same pass: the u64 rows A [rows][n] ++ B [rows], the u32 or u16 padded rows
// of ksk_width(n) (A, B at column n; the padding was zeroed by the caller).
struct KgKsk {
    uint64_t seed, qk;
    uint32_t rows, n, bKS, dKS, pow2, W;
    const uint64_t *sv, *svN, *dig;
    uint64_t* wksk;   // A [rows][n] ++ B [rows]
    uint32_t* ksk32;  // rows of W (or null)
    uint16_t* ksk16;  // rows of W (or null)
};

__global__ void __launch_bounds__(256) k_kgw_ksk(KgKsk c, DggTable dg) {
    const uint32_t row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= c.rows) return;
    const uint64_t s0 = rng_state(c.seed, T_KSK, row), qk = c.qk;
    uint64_t acc = 0;
    for (uint32_t t = lane; t < c.n; t += 64) {
        const uint64_t v = draw_uniform(s0, t, qk);
        const uint64_t pr = v * c.sv[t];
        acc += c.pow2 ? pr : pr % qk;
        c.wksk[(size_t)row * c.n + t] = v;
        if (c.ksk32) c.ksk32[(size_t)row * c.W + t] = (uint32_t)v;
        if (c.ksk16) c.ksk16[(size_t)row * c.W + t] = (uint16_t)v;
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) {
        const uint32_t i = row / (c.bKS * c.dKS), j = (row / c.dKS) % c.bKS, kk = row % c.dKS;
        const uint64_t jd = ((uint64_t)j * c.dig[kk]) % qk;
        const uint64_t sj = c.svN[i] * jd;
        uint64_t b = draw_dgg(s0, c.n, qk, dg);
        b = (b + (c.pow2 ? sj & (qk - 1) : sj % qk)) % qk;
        b = (b + (c.pow2 ? acc & (qk - 1) : acc % qk)) % qk;
        c.wksk[(size_t)c.rows * c.n + row] = b;
        if (c.ksk32) c.ksk32[(size_t)row * c.W + c.n] = (uint32_t)b;
        if (c.ksk16) c.ksk16[(size_t)row * c.W + c.n] = (uint16_t)b;
    }
}

// ---- second layouts: the host packers of engine_keys.cpp (pack_ginx3 / pack_n2k), one thread per destination word
struct KgRepack {
    const void* src;   // resident d_bsk_ (u32 when narrow, else u64)
    uint32_t* dst;
    size_t total;      // destination words of this launch
    size_t dst_off;    // first destination word
    size_t src_off;    // first source word of the automorphism keys (ak kinds)
    uint64_t Q, c;     // destination = resident word * c mod Q
    uint32_t N, dG2, nd, narrow, kind;
};
enum : uint32_t { RP_G3_GINX, RP_G3_EK, RP_G3_AK, RP_N2K_GINX, RP_N2K_EK, RP_N2K_AK };

__global__ void __launch_bounds__(256) k_kg_repack(KgRepack a) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.total) return;
    const uint32_t N = a.N, dG2 = a.dG2;
    const uint32_t e = t & 3, L = (t >> 2) & 63;
    size_t src, dst;
    if (a.kind == RP_G3_GINX) {  // [i][c][p < 6][k2 < 8][64][4] (boot.h g2_key_word, nd = 3)
        const size_t i = t / 24576;
        const uint32_t r = (uint32_t)(t % 24576), k2 = (r >> 8) & 7, cp = r >> 11, c = cp / 6, p = cp % 6;
        const uint32_t rr = 2 * k2 + (e & 1), ks = e >> 1, x = ((rr >> 2) << 8) | (L << 2) | (rr & 3);
        src = (((i * 2 + ks) * dG2 + g2_row(c, p, 3)) * 2 + c) * N + x;
        dst = i * 24576 + g2_key_word(3, c, p, k2, L, e);
    } else if (a.kind == RP_G3_EK) {  // ek [i][c][p < 6][k4 < 4][64][4]
        const size_t i = t / 12288;
        const uint32_t r = (uint32_t)(t % 12288), k4 = (r >> 8) & 3, cp = r >> 10, c = cp / 6, p = cp % 6;
        const uint32_t x = (k4 << 8) | (L << 2) | e;
        src = ((i * dG2 + g2_row(c, p, 3)) * 2 + c) * N + x;
        dst = t;
    } else if (a.kind == RP_G3_AK) {  // ak [t][c][d < 3][k4][64][4]
        const size_t k = t / 6144;
        const uint32_t r = (uint32_t)(t % 6144), k4 = (r >> 8) & 3, cd = r >> 10, c = cd / 3, dd = cd % 3;
        const uint32_t x = (k4 << 8) | (L << 2) | e;
        src = a.src_off + ((k * 3 + dd) * 2 + c) * N + x;
        dst = t;
    } else if (a.kind == RP_N2K_GINX) {  // [i][c][q < kq][k2 < 16][64][4], kq = 2 nd
        const uint32_t kq = 2 * a.nd;
        const size_t per = (size_t)2 * kq * 4096, i = t / per;
        const uint32_t r = (uint32_t)(t % per), k2 = (r >> 8) & 15, cq = r >> 12, c = cq / kq, q = cq % kq;
        const uint32_t rr = 2 * k2 + (e & 1), ks = e >> 1, x = ((rr >> 1) << 7) | (L << 1) | (rr & 1);
        const uint32_t row = 2 * (q >> 1) + c, col = (q & 1) ? 1 - c : c;
        src = (((i * 2 + ks) * dG2 + row) * 2 + col) * N + x;
        dst = t;
    } else if (a.kind == RP_N2K_EK) {  // ek [i][c][q < kq][k4 < 8][64][4]
        const uint32_t kq = 2 * a.nd;
        const size_t per = (size_t)2 * kq * 2048, i = t / per;
        const uint32_t r = (uint32_t)(t % per), k4 = (r >> 8) & 7, cq = r >> 11, c = cq / kq, q = cq % kq;
        const uint32_t rr = 4 * k4 + e, x = ((rr >> 1) << 7) | (L << 1) | (rr & 1);
        const uint32_t row = 2 * (q >> 1) + c, col = (q & 1) ? 1 - c : c;
        src = ((i * dG2 + row) * 2 + col) * N + x;
        dst = t;
    } else {  // RP_N2K_AK: ak [t][q < kq][k4][64][4], q = 2 d + column
        const uint32_t kq = 2 * a.nd;
        const size_t aper = (size_t)kq * 2048, k = t / aper;
        const uint32_t r = (uint32_t)(t % aper), k4 = (r >> 8) & 7, q = r >> 11, d = q >> 1, col = q & 1;
        const uint32_t rr = 4 * k4 + e, x = ((rr >> 1) << 7) | (L << 1) | (rr & 1);
        src = a.src_off + ((k * a.nd + d) * 2 + col) * N + x;
        dst = t;
    }
    const uint64_t w = a.narrow ? static_cast<const uint32_t*>(a.src)[src] : static_cast<const uint64_t*>(a.src)[src];
    a.dst[a.dst_off + dst] = (uint32_t)((w * a.c) % a.Q);  // w, c < Q < 2^32
}

inline int64_t signed_of(uint64_t x, uint64_t m) { return x > (m >> 1) ? (int64_t)x - (int64_t)m : (int64_t)x; }
inline uint64_t lift(int64_t v, uint64_t m) {
    const int64_t r = v % (int64_t)m;
    return (uint64_t)(r < 0 ? r + (int64_t)m : r);
}

template <class T>
struct Tmp {
    T* p = nullptr;
    explicit Tmp(size_t count) { FHE_HIP_CHECK(hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T))); }
    ~Tmp() { (void)hipFree(p); }
    Tmp(const Tmp&) = delete;
    Tmp& operator=(const Tmp&) = delete;
};

}  // namespace

void keygen_bootstrap_device_wide(const Params& p, const std::vector<uint64_t>& sk, uint64_t seed, int device,
                                  const KgWideOut& out, void* stream) {
    if (sk.size() != p.n) throw std::invalid_argument("secret key has wrong length");
    for (uint64_t v : sk)
        if (v >= p.qKS) throw std::invalid_argument("secret key not reduced mod qKS");
    if (const char* why = ntt_plan_check(p.Q, p.N))
        throw std::invalid_argument(std::string("device key generation: no transform for (Q, N): ") + why);
    const uint32_t n = p.n, N = p.N;
    const uint64_t Q = p.Q, qk = p.qKS;
    const bool pow2ks = !(qk & (qk - 1));
    if (!pow2ks && qk >= (1ull << 32)) throw std::invalid_argument("device key generation expects qKS a power of two or below 2^32");
    if (out.narrow && Q >= (1ull << 32)) throw std::invalid_argument("device key generation: 32-bit key words need Q < 2^32");
    hipStream_t s = static_cast<hipStream_t>(stream);
    FHE_HIP_CHECK(hipSetDevice(device));

    // ring secret, its EVALUATION form and the permuted secrets (host: N coefficients each), times R = 2^64
    std::vector<uint64_t> skN, S;
    keygen_ring_secret(p, seed, skN);
    S = skN;
    HostNtt ntt;
    ntt.init(N, Q, p.psi);
    ntt.forward(S.data());
    std::vector<KgRow> desc;
    keygen_descriptors(p, sk.data(), seed, desc);
    std::vector<uint64_t> skAuto;
    if (p.method == M_LMKCDEY) {
        skAuto.resize((size_t)(p.numAutoKeys + 1) * N);
        for (uint32_t k = 0; k <= p.numAutoKeys; ++k) {
            const uint32_t kk = k == 0 ? 2 * N - 5 : (uint32_t)powmod(5, k, 2 * N);
            auto_eval(p, kk, S.data(), skAuto.data() + (size_t)k * N);
        }
    }
    const uint64_t R = (uint64_t)(((u128)1 << 64) % Q);
    for (uint64_t& v : S) v = mulmod(v, R, Q);
    for (uint64_t& v : skAuto) v = mulmod(v, R, Q);
    uint64_t inv = Q;  // Q^-1 mod 2^64 (Newton)
    for (int i = 0; i < 6; ++i) inv *= 2 - Q * inv;

    Tmp<KgRow> dd(desc.size());
    Tmp<uint64_t> dS(N), dAuto(skAuto.size());
    FHE_HIP_CHECK(hipMemcpyAsync(dd.p, desc.data(), desc.size() * sizeof(KgRow), hipMemcpyHostToDevice, s));
    FHE_HIP_CHECK(hipMemcpyAsync(dS.p, S.data(), N * 8, hipMemcpyHostToDevice, s));
    if (!skAuto.empty())
        FHE_HIP_CHECK(hipMemcpyAsync(dAuto.p, skAuto.data(), skAuto.size() * 8, hipMemcpyHostToDevice, s));
    NttPlan plan;
    FHE_HIP_CHECK(ntt_plan_init(plan, Q, p.psi, N, device));
    struct PlanGuard { NttPlan& p; ~PlanGuard() { ntt_plan_free(p); } } guard{plan};
    const size_t chunk = keygen_chunk_pairs(N, desc.size());  // A / [E, M] scratch capped at kKgScratchCap
    Tmp<uint64_t> dA(chunk * N), dT(chunk * 2 * N);
    KgFinish f{Q, 0 - inv, mulmod(R, R, Q), dS.p, dAuto.p, out.bsk, out.raw_bsk, N, out.narrow ? 1u : 0u};
    for (size_t c0 = 0; c0 < desc.size(); c0 += chunk) {
        const uint32_t nc = (uint32_t)std::min(chunk, desc.size() - c0);
        k_kgw_sample<<<nc, 256, 0, s>>>(dd.p + c0, N, Q, dA.p, dT.p, dgg_table());
        FHE_HIP_CHECK(hipGetLastError());
        FHE_HIP_CHECK(ntt_launch(plan, dT.p, dT.p, 2 * nc, false, s));
        k_kgw_finish<<<nc, 256, 0, s>>>(dd.p + c0, dA.p, dT.p, f);
        FHE_HIP_CHECK(hipGetLastError());
    }

    // key-switching key
    const uint32_t rows = (uint32_t)p.ksk_rows();
    const uint32_t W = ksk_width(n);
    std::vector<uint64_t> sv(W, 0), svN(N), dig(p.digitsKS);
    for (uint32_t i = 0; i < n; ++i) sv[i] = sk[i] % qk;
    for (uint32_t i = 0; i < N; ++i) svN[i] = lift(signed_of(skN[i], Q), qk);
    {
        uint64_t v = 1;
        for (uint32_t k = 0; k < p.digitsKS; ++k, v *= p.baseKS) dig[k] = v;
    }
    Tmp<uint64_t> dsv(W), dsvN(N), ddig(dig.size());
    FHE_HIP_CHECK(hipMemcpyAsync(dsv.p, sv.data(), W * 8, hipMemcpyHostToDevice, s));
    FHE_HIP_CHECK(hipMemcpyAsync(dsvN.p, svN.data(), N * 8, hipMemcpyHostToDevice, s));
    FHE_HIP_CHECK(hipMemcpyAsync(ddig.p, dig.data(), dig.size() * 8, hipMemcpyHostToDevice, s));
    KgKsk c{seed, qk, rows, n, p.baseKS, p.digitsKS, pow2ks ? 1u : 0u, W, dsv.p, dsvN.p, ddig.p, out.wksk, out.ksk32, out.ksk16};
    k_kgw_ksk<<<(rows + 3) / 4, 256, 0, s>>>(c, dgg_table());
    FHE_HIP_CHECK(hipGetLastError());
    FHE_HIP_CHECK(hipStreamSynchronize(s));  // temporaries are freed on return
}

void keygen_repack_device(const Params& p, bool g3, bool narrow, const void* d_bsk, uint32_t* d_bsk2, void* stream) {
    const uint32_t n = p.n, N = p.N, dG2 = p.digitsG2, nd = p.digitsG - 1;
    const uint64_t Q = p.Q;
    if (Q >= (1ull << 32)) throw std::invalid_argument("device key repack expects Q < 2^32");
    const bool lmk = p.method == M_LMKCDEY;
    const size_t nauto = lmk ? (size_t)p.numAutoKeys + 1 : 0;
    // destination to_mont(x N^-1) = x N^-1 2^32: the resident word x 2^32 (narrow) times N^-1, or x 2^64 times N^-1 2^-32
    const uint64_t ninv = invmod(N, Q);
    const uint64_t c = narrow ? ninv : mulmod(ninv, invmod((1ull << 32) % Q, Q), Q);
    hipStream_t s = static_cast<hipStream_t>(stream);
    KgRepack a{d_bsk, d_bsk2, 0, 0, (size_t)n * dG2 * 2 * N, Q, c, N, dG2, nd, narrow ? 1u : 0u, 0};
    auto run = [&](uint32_t kind, size_t total, size_t dst_off) {
        a.kind = kind;
        a.total = total;
        a.dst_off = dst_off;
        if (!total) return;
        k_kg_repack<<<(unsigned)((total + 255) / 256), 256, 0, s>>>(a);
        FHE_HIP_CHECK(hipGetLastError());
    };
    const KgRepackSizes z = keygen_repack_sizes(p, g3);
    if (g3) {
        run(lmk ? RP_G3_EK : RP_G3_GINX, (size_t)n * z.per, 0);
        if (lmk) run(RP_G3_AK, nauto * z.aper, (size_t)n * z.per);
    } else {
        run(lmk ? RP_N2K_EK : RP_N2K_GINX, (size_t)n * z.per, 0);
        if (lmk) run(RP_N2K_AK, nauto * z.aper, (size_t)n * z.per);
    }
}

}  // namespace fhe_amd
