// pke.hip -- the public-key side of LWEEncryptionScheme on the device: PubKeyGen (lwe-pke.cpp:74-98) and
// EncryptN (lwe-pke.cpp:133-167).  Bit-identical to the host generator (keygen.cpp pubkey_gen / encrypt_pk)
// for the same seed: every draw of the counter generator is computed independently here (keygen.h).
//
//   k_pk_gen       one wave per row j of A: N uniform draws written to the resident key, <A[j], s> by wave
//                  reduction, v[j] = e_j + <A[j], s>
//   k_pk_draw      the ternary s' of every ciphertext, 2 bits each, [N / 16][count] words (read coalesced by
//                  the two kernels below, once per 16 rows)
//   k_encrypt_pk   a = e' + s'^T A.  A workgroup owns kPkTileG ciphertexts x kPkTileC columns; kPkTileR rows
//                  of that column slice of A are staged in LDS, double-buffered; one thread per ciphertext
//                  keeps its column sums in registers and adds, subtracts or skips row j by its own s'_j.
//                  All lanes read the same LDS address (16-byte reads): a broadcast, no bank conflicts.
//   k_encrypt_pk_b b = (m mod p) floor(Q / p) + e'' + <v, s'>, one thread per ciphertext
//
// Exactness.  Word = u32 (Q < 2^31): the sums are signed 64-bit, unreduced: |e'| + N max|A| < 40 + 2^11 2^31 <
// 2^43, reduced mod Q once at the end (quotient estimated in double precision, which holds the sum exactly, then
// corrected by at most one Q either way).  Word = u64 (Q < 2^56): the sums stay in [0, Q); each step adds
// x, Q - x or 0 (at most Q) and subtracts Q once when the sum reaches it, so nothing passes 2 Q < 2^57.
#include <hip/hip_runtime.h>

#include "pke.h"
#include "rng_dev.h"

namespace fhe_amd {
namespace {

constexpr uint32_t kSkip = 0x55555555u;  // sixteen packed s' = 0

template <class Word>
__global__ void __launch_bounds__(256) k_pk_gen(uint64_t seed, uint32_t N, uint64_t Q, const int32_t* __restrict__ s,
                                                Word* __restrict__ A, uint64_t* __restrict__ v,
                                                uint64_t* __restrict__ rawA, DggTable dg) {
    const uint32_t row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= N) return;
    const uint64_t s0 = rng_state(seed, T_PKA, row);
    uint64_t acc = 0;
    for (uint32_t i = lane; i < N; i += 64) {
        const uint64_t x = draw_uniform(s0, i, Q);
        A[(size_t)row * N + i] = (Word)x;
        if (rawA) rawA[(size_t)row * N + i] = x;
        const int32_t si = s[i];                                   // |s_i| <= kDggMaxFin: x |s_i| < 2^62
        uint64_t t = (x * (uint64_t)(si < 0 ? -si : si)) % Q;
        if (si < 0 && t) t = Q - t;
        acc += t;
        acc = acc >= Q ? acc - Q : acc;
    }
    for (int o = 32; o > 0; o >>= 1) {
        acc += __shfl_xor(acc, o, 64);
        acc = acc >= Q ? acc - Q : acc;
    }
    if (lane == 0) {
        const uint64_t e = draw_dgg(rng_state(seed, T_PKV, 0), row, Q, dg);
        acc += e;
        v[row] = acc >= Q ? acc - Q : acc;
    }
}

__global__ void __launch_bounds__(256) k_pk_draw(uint64_t seed, uint64_t first, uint32_t count,
                                                 uint32_t* __restrict__ sp) {
    const uint32_t g = blockIdx.x * 256 + threadIdx.x, w = blockIdx.y;
    if (g >= count) return;
    const uint64_t s0 = rng_state(seed, T_PKENC, first + g);
    uint32_t word = 0;
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) word |= (uint32_t)draw_uniform(s0, w * 16 + k, 3) << (2 * k);
    sp[(size_t)w * count + g] = word;
}

__global__ void __launch_bounds__(256) k_encrypt_pk_b(uint64_t seed, uint64_t first, uint32_t N, uint64_t Q,
                                                      uint32_t ptmod, const uint64_t* __restrict__ v,
                                                      const int32_t* __restrict__ bits,
                                                      const uint32_t* __restrict__ sp, uint32_t count,
                                                      uint64_t* __restrict__ b_out, DggTable dg) {
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    if (g >= count) return;
    const uint64_t s0 = rng_state(seed, T_PKENC, first + g);
    uint64_t acc = ((uint64_t)((uint32_t)bits[g] % ptmod) * (Q / ptmod)) % Q;
    acc += draw_dgg(s0, 2 * (uint64_t)N, Q, dg);
    acc = acc >= Q ? acc - Q : acc;
    for (uint32_t w = 0; w < N / 16; ++w) {
        const uint32_t word = sp[(size_t)w * count + g];
#pragma unroll
        for (uint32_t k = 0; k < 16; ++k) {
            const uint32_t t = (word >> (2 * k)) & 3;   // s' + 1
            const uint64_t x = v[w * 16 + k];
            acc += t == 2 ? x : t == 0 ? Q - x : 0;
            acc = acc >= Q ? acc - Q : acc;
        }
    }
    b_out[g] = acc;
}

template <class Word>
struct PkSum;
template <>
struct PkSum<uint32_t> {
    using T = int64_t;
    using Vec = uint4;  // one 16-byte LDS read
    static constexpr uint32_t kPer = 4;
    static __device__ __forceinline__ T init(uint64_t s0, uint64_t k, uint64_t, const DggTable& dg) {
        return dgg_sample(draw(s0, k), dg);
    }
    static __device__ __forceinline__ void step(T* acc, const Vec& x, int32_t s, uint64_t) {
        acc[0] += (int64_t)s * (int32_t)x.x;
        acc[1] += (int64_t)s * (int32_t)x.y;
        acc[2] += (int64_t)s * (int32_t)x.z;
        acc[3] += (int64_t)s * (int32_t)x.w;
    }
    static __device__ __forceinline__ uint64_t fin(T acc, uint64_t Q, double inv) {
        const int64_t q = (int64_t)floor((double)acc * inv);
        int64_t r = acc - q * (int64_t)Q;
        r = r < 0 ? r + (int64_t)Q : r;
        r = r >= (int64_t)Q ? r - (int64_t)Q : r;
        return (uint64_t)r;
    }
};
template <>
struct PkSum<uint64_t> {
    using T = uint64_t;
    using Vec = ulonglong2;
    static constexpr uint32_t kPer = 2;
    static __device__ __forceinline__ T init(uint64_t s0, uint64_t k, uint64_t Q, const DggTable& dg) {
        return draw_dgg(s0, k, Q, dg);
    }
    static __device__ __forceinline__ void one(T& acc, uint64_t x, int32_t s, uint64_t Q) {
        acc += s > 0 ? x : s < 0 ? Q - x : 0;
        acc = acc >= Q ? acc - Q : acc;
    }
    static __device__ __forceinline__ void step(T* acc, const Vec& x, int32_t s, uint64_t Q) {
        one(acc[0], x.x, s, Q);
        one(acc[1], x.y, s, Q);
    }
    static __device__ __forceinline__ uint64_t fin(T acc, uint64_t, double) { return acc; }
};

template <class Word>
__global__ void __launch_bounds__(kPkTileG) k_encrypt_pk(uint64_t seed, uint64_t first, uint32_t N, uint64_t Q,
                                                         const Word* __restrict__ A, const uint32_t* __restrict__ sp,
                                                         uint32_t count, uint64_t* __restrict__ a_out, DggTable dg) {
    using S = PkSum<Word>;
    constexpr uint32_t G = kPkTileG, C = kPkTileC, R = kPkTileR, TW = R * C, LD = TW / G;
    static_assert(TW % G == 0 && R % 16 == 0 && C % S::kPer == 0, "tile shape");
    __shared__ __attribute__((aligned(16))) Word tile[2][TW];
    const uint32_t tid = threadIdx.x, g = blockIdx.x * G + tid, c0 = blockIdx.y * C;
    const bool live = g < count;
    const uint64_t s0 = rng_state(seed, T_PKENC, first + g);

    typename S::T acc[C];
#pragma unroll
    for (uint32_t c = 0; c < C; ++c) acc[c] = S::init(s0, (uint64_t)N + c0 + c, Q, dg);  // e'

    Word pre[LD];
    auto fetch = [&](uint32_t j0) {
#pragma unroll
        for (uint32_t l = 0; l < LD; ++l) {
            const uint32_t k = tid + l * G;
            pre[l] = A[(size_t)(j0 + k / C) * N + c0 + k % C];
        }
    };
    auto stash = [&](uint32_t buf) {
#pragma unroll
        for (uint32_t l = 0; l < LD; ++l) tile[buf][tid + l * G] = pre[l];
    };
    fetch(0);
    stash(0);
    __syncthreads();
    for (uint32_t j0 = 0, buf = 0; j0 < N; j0 += R, buf ^= 1) {
        const bool more = j0 + R < N;
        if (more) fetch(j0 + R);
        for (uint32_t h = 0; h < R / 16; ++h) {
            const uint32_t word = live ? sp[(size_t)((j0 >> 4) + h) * count + g] : kSkip;
#pragma unroll
            for (uint32_t k = 0; k < 16; ++k) {
                const int32_t s = (int32_t)((word >> (2 * k)) & 3) - 1;
                const Word* row = &tile[buf][(h * 16 + k) * C];
#pragma unroll
                for (uint32_t c = 0; c < C; c += S::kPer)
                    S::step(acc + c, *reinterpret_cast<const typename S::Vec*>(row + c), s, Q);
            }
        }
        if (more) stash(buf ^ 1);
        __syncthreads();
    }
    if (!live) return;
    const double inv = 1.0 / (double)Q;
#pragma unroll
    for (uint32_t c = 0; c < C; ++c) a_out[(size_t)g * N + c0 + c] = S::fin(acc[c], Q, inv);
}

}  // namespace

hipError_t launch_pk_gen(uint64_t seed, uint32_t N, uint64_t Q, const int32_t* d_s, void* d_key, uint64_t* raw_A,
                         hipStream_t s) {
    if (N == 0 || N % 64 || Q >= (1ull << 56)) return hipErrorInvalidValue;
    uint64_t* v = static_cast<uint64_t*>(d_key);
    if (pk_word32(Q))
        k_pk_gen<uint32_t><<<N / 4, 256, 0, s>>>(seed, N, Q, d_s, reinterpret_cast<uint32_t*>(v + N), v, raw_A,
                                                 dgg_table());
    else
        k_pk_gen<uint64_t><<<N / 4, 256, 0, s>>>(seed, N, Q, d_s, v + N, v, raw_A, dgg_table());
    return hipGetLastError();
}

hipError_t launch_encrypt_pk(uint64_t seed, uint64_t first, uint32_t N, uint64_t Q, uint32_t ptmod, const void* d_key,
                             const int32_t* d_bits, size_t count, uint32_t* d_sp, uint64_t* a_out, uint64_t* b_out,
                             hipStream_t s) {
    if (count == 0) return hipSuccess;
    if (N == 0 || N % kPkTileR || N % kPkTileC || Q >= (1ull << 56) || count > 0x7fffffffull || ptmod < 2)
        return hipErrorInvalidValue;
    const uint32_t cnt = (uint32_t)count;
    const uint64_t* v = static_cast<const uint64_t*>(d_key);
    k_pk_draw<<<dim3((cnt + 255) / 256, N / 16), 256, 0, s>>>(seed, first, cnt, d_sp);
    const dim3 grid((cnt + kPkTileG - 1) / kPkTileG, N / kPkTileC);
    if (pk_word32(Q))
        k_encrypt_pk<uint32_t><<<grid, kPkTileG, 0, s>>>(seed, first, N, Q, reinterpret_cast<const uint32_t*>(v + N),
                                                         d_sp, cnt, a_out, dgg_table());
    else
        k_encrypt_pk<uint64_t><<<grid, kPkTileG, 0, s>>>(seed, first, N, Q, v + N, d_sp, cnt, a_out, dgg_table());
    k_encrypt_pk_b<<<(cnt + 255) / 256, 256, 0, s>>>(seed, first, N, Q, ptmod, v, d_bits, d_sp, cnt, b_out,
                                                     dgg_table());
    return hipGetLastError();
}

}  // namespace fhe_amd
