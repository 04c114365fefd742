// ntt_sizes.hip -- batched negacyclic NTT / iNTT for every power-of-two N in 4 .. 65536 except the
// N = 1024 kernels of ntt.hip, and the pointwise product of the negacyclic multiply, for gfx950.
//
// Same transform as ntt.hip: the reference's ForwardTransformToBitReverseInPlace
// (transformnat-impl.h:302-373) and InverseTransformFromBitReverseInPlace (:511-624, N^-1 folded
// into the last stage), canonical u64 words in and out.  All arithmetic is exact mod Q, so the
// stage grouping below gives the reference's bits.
//
// One kernel, k_ntt_stages, runs a consecutive range of butterfly stages on a tile of E = 2^logE
// elements held in LDS, up to three stages per LDS round trip (radix 8 in registers).  Stage with
// half-length t of an N-point transform pairs (x, x + t) with the twiddle Table[N/(2t) + x/(2t)]
// = Table[(N + x) >> (log2 t + 1)].  Two launch shapes use it:
//   block mode:  the tile is E consecutive words of the batch (one polynomial, a contiguous block
//                of one, or several whole polynomials when N < E); stages t = B/2 .. 1 of blocks
//                of B words.  B = N is the whole transform in one pass.
//   column mode: N = R x B.  The first log2 R forward stages only couple the R words x = c + B j
//                of a column c, and their twiddle depends on j alone: an R-point transform with
//                Table[1 .. R-1].  The tile is R rows x W consecutive columns (row segments of W
//                words are contiguous, so loads and stores coalesce), and in tile coordinates
//                l = j W + c the stage is again (l, l + t) with Table[(E + l) >> (log2 t + 1)].
// Forward two-pass = column mode then block mode; inverse = block mode then column mode, whose
// last stage (twiddle index 1) carries the N^-1 fold.  Words between the passes are canonical.
//
// Two arithmetic widths, Harvey-lazy around Shoup's lazy product as in ntt.hip: 32-bit residues
// for Q < 2^30 (4Q < 2^32) and 64-bit residues for Q < 2^62 (4Q < 2^64).  Forward values live in
// [0, 4Q), inverse values in [0, 2Q); one correction on the way out gives [0, Q).
#include "arith.h"
#include "ntt.h"

namespace fhe_amd {

namespace {

constexpr uint32_t kLogTileMin = 11;  // a workgroup holds at least 2048 words: 2048 / N polynomials when N is smaller
constexpr uint32_t kLogOnePassMax = 14;  // 16384 u64 words + padding = 132 KiB of the 160 KiB LDS

FHE_DEV uint32_t lazy_mul(uint32_t x, uint2 w, uint32_t Q) { return mul_shoup_lazy(x, w.x, w.y, Q); }
FHE_DEV uint64_t lazy_mul(uint64_t x, ulonglong2 w, uint64_t Q) { return x * w.x - __umul64hi(x, w.y) * Q; }
FHE_DEV uint32_t cs(uint32_t x, uint32_t m) { return csub(x, m); }
FHE_DEV uint64_t cs(uint64_t x, uint64_t m) { return x >= m ? x - m : x; }

template <typename T> struct TwOf;
template <> struct TwOf<uint32_t> { using type = uint2; };
template <> struct TwOf<uint64_t> { using type = ulonglong2; };

// Shoup's lazy product x w - floor(x w' / beta) Q is in [0, 2Q) for any x < beta (beta = 2^32 or 2^64)
template <typename T>
struct LazyMod {
    using TW = typename TwOf<T>::type;  // (w, w' = floor(w beta / Q))
    T Q, Q2;
    TW lo, hi;  // (N^-1, pre), (TableI[1] N^-1, pre)
    // CT: (x, y) in [0,4Q)^2 -> (x + wy, x - wy) in [0,4Q)^2
    FHE_DEV void ct(T& x, T& y, TW w) const {
        x = cs(x, Q2);
        const T t = lazy_mul(y, w, Q);
        y = x + Q2 - t;
        x = x + t;
    }
    // GS: (x, y) in [0,2Q)^2 -> (x + y, (x - y) w) in [0,2Q)^2
    FHE_DEV void gs(T& x, T& y, TW w) const {
        const T d = x + Q2 - y;
        x = cs(x + y, Q2);
        y = lazy_mul(d, w, Q);
    }
    // last inverse stage: ((x + y) N^-1, (x - y) TableI[1] N^-1) in [0,2Q)
    FHE_DEV void gs_last(T& x, T& y) const {
        const T d = x + Q2 - y;
        x = lazy_mul(x + y, lo, Q);
        y = lazy_mul(d, hi, Q);
    }
    FHE_DEV T fwd_out(T x) const { return cs(cs(x, Q2), Q); }
    FHE_DEV T inv_out(T x) const { return cs(x, Q); }
};

struct StageArgs {
    uint32_t logE;     // words per workgroup
    uint32_t logNv;    // twiddle index space: log2 N (block mode) or logE (column mode)
    uint32_t logT0;    // log2 of the first stage's half-length, in tile coordinates
    uint32_t nstages;
    uint32_t logW;     // column mode: log2 of the tile's width; block mode: logE (one row)
    uint32_t logB;     // column mode: log2 of the row stride B
    uint32_t logN;
    uint32_t cols;     // column mode
    uint64_t total;    // count * N words
};

// one 32-word bank row of padding per 32 words: the strided accesses of a radix-8 group (words
// X + e tl, tl a power of two) spread over the banks
FHE_DEV uint32_t pad(uint32_t x) { return x + (x >> 5); }

// K stages on the tile in LDS.  A thread takes the 2^K words X + e tl (e = 0 .. 2^K - 1, X with
// those K bits clear), tl = the smallest half-length of the K stages, and runs the stage of bit b
// of e on the pairs (e, e | 1 << b): forward from the top bit down, inverse from bit 0 up.
// Stage bit b has 2^(K-1-b) distinct twiddles in the group, at consecutive table indices.
template <typename T, bool INV, int K>
FHE_DEV void round_k(T* s, const typename TwOf<T>::type* __restrict__ tab, const LazyMod<T>& m,
                     uint32_t logE, uint32_t ltl, uint32_t logNv, uint32_t xoff) {
    using TW = typename TwOf<T>::type;
    const uint32_t Nv = 1u << logNv;
    for (uint32_t g = threadIdx.x; g < (1u << (logE - K)); g += blockDim.x) {
        const uint32_t X = ((g >> ltl) << (ltl + K)) | (g & ((1u << ltl) - 1));
        const uint32_t xt = Nv + ((xoff + X) & (Nv - 1));
        T v[1 << K];
#pragma unroll
        for (int e = 0; e < (1 << K); ++e) v[e] = s[pad(X + ((uint32_t)e << ltl))];
#pragma unroll
        for (int st = 0; st < K; ++st) {
            const int b       = INV ? st : K - 1 - st;
            const uint32_t sh = ltl + b + 1;
            const bool last   = INV && sh == logNv;  // twiddle index 1: the N^-1 fold
            TW w[1 << (K - 1)];
            if (!last) {
#pragma unroll
                for (int h = 0; h < (1 << (K - 1 - b)); ++h) w[h] = tab[(xt >> sh) + h];
            }
#pragma unroll
            for (int e = 0; e < (1 << K); ++e) {
                if (e & (1 << b)) continue;
                if (!INV) m.ct(v[e], v[e | (1 << b)], w[e >> (b + 1)]);
                else if (last) m.gs_last(v[e], v[e | (1 << b)]);
                else m.gs(v[e], v[e | (1 << b)], w[e >> (b + 1)]);
            }
        }
#pragma unroll
        for (int e = 0; e < (1 << K); ++e) s[pad(X + ((uint32_t)e << ltl))] = v[e];
    }
}

template <typename T, bool INV>
__global__ void __launch_bounds__(1024)
    k_ntt_stages(const uint64_t* in, uint64_t* out,  // in may be out: a workgroup reads its tile, then writes it
                 const typename TwOf<T>::type* __restrict__ tab, LazyMod<T> m, StageArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    T* s             = reinterpret_cast<T*>(smem);
    const uint32_t E = 1u << a.logE;
    size_t gbase;
    uint32_t xoff, nvalid;
    if (a.cols) {
        const uint32_t lt = a.logB - a.logW;  // tiles per polynomial
        gbase  = ((size_t)(blockIdx.x >> lt) << a.logN) + ((size_t)(blockIdx.x & ((1u << lt) - 1)) << a.logW);
        xoff   = 0;
        nvalid = E;
    } else {
        gbase  = (size_t)blockIdx.x << a.logE;
        xoff   = (uint32_t)(gbase & ((1u << a.logN) - 1));
        nvalid = a.total - gbase < E ? (uint32_t)(a.total - gbase) : E;  // whole polynomials (N < E) or E
    }
    auto gaddr = [&](uint32_t l) -> size_t {
        return gbase + ((size_t)(l >> a.logW) << a.logB) + (l & ((1u << a.logW) - 1));
    };
    for (uint32_t l = threadIdx.x; l < E; l += blockDim.x) s[pad(l)] = l < nvalid ? (T)in[gaddr(l)] : (T)0;
    __syncthreads();
    for (uint32_t done = 0; done < a.nstages;) {
        const uint32_t K = a.nstages - done < 3 ? a.nstages - done : 3;
        // the smallest half-length of this round's stages
        const uint32_t ltl = INV ? a.logT0 + done : a.logT0 - done - (K - 1);
        if (K == 3) round_k<T, INV, 3>(s, tab, m, a.logE, ltl, a.logNv, xoff);
        else if (K == 2) round_k<T, INV, 2>(s, tab, m, a.logE, ltl, a.logNv, xoff);
        else round_k<T, INV, 1>(s, tab, m, a.logE, ltl, a.logNv, xoff);
        __syncthreads();
        done += K;
    }
    for (uint32_t l = threadIdx.x; l < nvalid; l += blockDim.x)
        out[gaddr(l)] = (uint64_t)(INV ? m.inv_out(s[pad(l)]) : m.fwd_out(s[pad(l)]));
}

// out = a b mod Q on canonical words, any odd Q < 2^63: two Montgomery reductions (R = 2^64),
// a b R^-1 and then (a b R^-1) R^2 R^-1.  qinv = Q^-1 mod 2^64, r2 = 2^128 mod Q.
FHE_DEV uint64_t mont64(uint64_t a, uint64_t b, uint64_t Q, uint64_t qinv) {
    const uint64_t lo = a * b, hi = __umul64hi(a, b);  // a b < Q 2^64, so hi < Q
    const uint64_t mq = __umul64hi(lo * qinv, Q);      // (a b - (lo qinv) Q) / 2^64 = hi - mq in (-Q, Q)
    return hi >= mq ? hi - mq : hi + Q - mq;
}
__global__ void __launch_bounds__(256)
    k_pointwise_mul(const uint64_t* a, const uint64_t* b, uint64_t* out,  // out may be a or b
                    size_t n, uint64_t Q, uint64_t qinv, uint64_t r2) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        out[i] = mont64(mont64(a[i], b[i], Q, qinv), r2, Q, qinv);
}

struct Shape {
    uint32_t passes, logR, logB;  // N = 2^logR x 2^logB; one pass: logR = 0
};
Shape shape_of(uint32_t logN, uint32_t log_onepass) {
    if (logN <= log_onepass) return {1, 0, logN};
    // R = 8 or 64: whole radix-8 rounds in the column pass.  log_onepass >= 11 and logN <= 16, so
    // R = 64 always leaves blocks that fit one pass.
    const uint32_t logR = logN - 3 <= log_onepass ? 3 : 6;
    return {2, logR, logN - logR};
}

template <typename T>
hipError_t launch_stages(const NttPlan& p, const uint64_t* in, uint64_t* out, const StageArgs& a, uint64_t groups,
                         bool inverse, hipStream_t s) {
    using TW = typename TwOf<T>::type;
    if (groups > 0x7fffffffull) return hipErrorInvalidValue;
    const uint32_t E = 1u << a.logE;
    uint32_t threads = E / 8;
    threads          = threads < 256 ? 256 : threads > 1024 ? 1024 : threads;
    const size_t sm  = (size_t)(E + E / 32) * sizeof(T);
    const TW* tab    = reinterpret_cast<const TW*>(inverse ? p.d_tab_inv : p.d_tab_fwd);
    LazyMod<T> m;
    m.Q  = (T)p.Q;
    m.Q2 = (T)(2 * p.Q);
    m.lo = TW{(T)p.ninv, (T)p.ninv_pre};
    m.hi = TW{(T)p.w1ninv, (T)p.w1ninv_pre};
    if (inverse) hipLaunchKernelGGL((k_ntt_stages<T, true>), dim3((uint32_t)groups), dim3(threads), sm, s, in, out, tab, m, a);
    else hipLaunchKernelGGL((k_ntt_stages<T, false>), dim3((uint32_t)groups), dim3(threads), sm, s, in, out, tab, m, a);
    return hipGetLastError();
}

// stages t = B/2 .. 1 (forward) or 1 .. B/2 (inverse) of every block of B = 2^logB consecutive words
template <typename T>
hipError_t launch_blocks(const NttPlan& p, const uint64_t* in, uint64_t* out, uint32_t count, uint32_t logN,
                         uint32_t logB, bool inverse, hipStream_t s) {
    StageArgs a{};
    a.logE    = logB < kLogTileMin ? kLogTileMin : logB;
    a.logNv   = logN;
    a.logT0   = inverse ? 0 : logB - 1;
    a.nstages = logB;
    a.logW    = a.logE;
    a.logB    = 0;
    a.logN    = logN;
    a.cols    = 0;
    a.total   = (uint64_t)count << logN;
    return launch_stages<T>(p, in, out, a, (a.total + (1ull << a.logE) - 1) >> a.logE, inverse, s);
}

// the R = 2^logR point transforms over the columns c + B j: tiles of R rows x 2048 / R columns
template <typename T>
hipError_t launch_columns(const NttPlan& p, const uint64_t* in, uint64_t* out, uint32_t count, uint32_t logN,
                          uint32_t logR, bool inverse, hipStream_t s) {
    StageArgs a{};
    a.logE    = kLogTileMin;
    a.logNv   = a.logE;
    a.logW    = a.logE - logR;
    a.logB    = logN - logR;
    a.logT0   = inverse ? a.logW : a.logE - 1;
    a.nstages = logR;
    a.logN    = logN;
    a.cols    = 1;
    a.total   = (uint64_t)count << logN;
    return launch_stages<T>(p, in, out, a, (uint64_t)count << (a.logB - a.logW), inverse, s);
}

template <typename T>
hipError_t launch_sizes(const NttPlan& p, const uint64_t* in, uint64_t* out, uint32_t count, bool inverse,
                        hipStream_t s) {
    uint32_t logN = 0;
    while ((1u << logN) < p.N) ++logN;
    const Shape sh = shape_of(logN, p.log_onepass);
    if (sh.passes == 1) return launch_blocks<T>(p, in, out, count, logN, logN, inverse, s);
    hipError_t e;
    if (!inverse) {
        if ((e = launch_columns<T>(p, in, out, count, logN, sh.logR, false, s)) != hipSuccess) return e;
        return launch_blocks<T>(p, out, out, count, logN, sh.logB, false, s);
    }
    if ((e = launch_blocks<T>(p, in, out, count, logN, sh.logB, true, s)) != hipSuccess) return e;
    return launch_columns<T>(p, out, out, count, logN, sh.logR, true, s);
}

}  // namespace

// The `cut` rows of profiles/ntt_sizes_time.txt run N = 8192 and N = 16384 both ways: one pass is the
// faster at both sizes and in both widths, even with one 1024-thread workgroup per CU at 16384.  So
// both widths stay in one pass up to the largest tile that fits LDS, and the width does not move the
// cut today (callers still ask per width: a u32 tile is half a u64 tile's bytes).
uint32_t ntt_onepass_default(bool wide) {
    (void)wide;
    return 1u << kLogOnePassMax;
}

bool ntt_onepass_valid(uint32_t n) {
    return n >= (1u << kLogTileMin) && n <= (1u << kLogOnePassMax) && (n & (n - 1)) == 0;
}

void ntt_dispatch_info(const NttPlan& p, uint32_t* passes, uint32_t* polys_per_group) {
    uint32_t logN = 0;
    while ((1u << logN) < p.N) ++logN;
    if (p.N == 1024) {  // ntt.hip: one polynomial per wave, 8 waves per workgroup
        *passes          = 1;
        *polys_per_group = 8;
        return;
    }
    *passes          = shape_of(logN, p.log_onepass).passes;
    *polys_per_group = logN < kLogTileMin ? 1u << (kLogTileMin - logN) : 1;
}

// the stage kernels stage up to 132 KiB per workgroup: above the 64 KiB a launch gets by default
hipError_t ntt_sizes_prepare() {
    const int bytes      = (int)(((1u << kLogOnePassMax) + (1u << kLogOnePassMax) / 32) * sizeof(uint64_t));
    const void* fns[4] = {reinterpret_cast<const void*>(&k_ntt_stages<uint32_t, false>),
                          reinterpret_cast<const void*>(&k_ntt_stages<uint32_t, true>),
                          reinterpret_cast<const void*>(&k_ntt_stages<uint64_t, false>),
                          reinterpret_cast<const void*>(&k_ntt_stages<uint64_t, true>)};
    for (const void* f : fns) {
        const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t ntt_launch(const NttPlan& p, const uint64_t* in, uint64_t* out, uint32_t count, bool inverse,
                      hipStream_t s) {
    if (p.N == 1024) return ntt1024_launch(p, in, out, count, inverse, s);
    if (count == 0) return hipSuccess;
    if (p.wide) return launch_sizes<uint64_t>(p, in, out, count, inverse, s);
    return launch_sizes<uint32_t>(p, in, out, count, inverse, s);
}

hipError_t ntt_pointwise_mul(const NttPlan& p, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t words,
                             hipStream_t s) {
    if (words == 0) return hipSuccess;
    const size_t groups = (words + 255) / 256, cap = (size_t)p.cus * 16;
    hipLaunchKernelGGL(k_pointwise_mul, dim3((uint32_t)(groups < cap ? groups : cap)), dim3(256), 0, s, a, b, out, words,
                       p.Q, p.qinv64, p.r2);
    return hipGetLastError();
}

}  // namespace fhe_amd
