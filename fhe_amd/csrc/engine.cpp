// engine.cpp -- see engine.h.
#include "engine.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "keygen.h"
#include "nt.h"

namespace fhe_amd {

bool Engine::fast_path(const Params& p) {
    const bool pow2q = !(p.q & (p.q - 1)), pow2ks = !(p.qKS & (p.qKS - 1));
    return !is_large(p.paramset) && p.N == 1024 && p.Q < (1ull << 28) && p.digitsG == 3 && pow2q && pow2ks &&
           p.qKS <= 65536 && p.n < 1024;
}

bool Engine::narrow_set(const Params& p) {
    // the 64-bit accumulator's 32-bit policy (bootstrap_wide.hip A32): residues and digit x key sums
    // (< digitsG2 Q^2 < Q 2^32) in 32-bit words
    return p.Q < (1ull << 30) && (uint64_t)p.digitsG2 * p.Q < (1ull << 32);
}

bool Engine::g3_set(const Params& p) {
    // digit fields of d + C in 32 bits (boot_arith.h decompose_n): 4 g <= 32 and C + Q < 2^32
    const uint64_t g = p.gBits, h = 1ull << (g - 1);
    const uint64_t C = h * (1 + (1ull << g) + (1ull << (2 * g)) + (1ull << (3 * g)));
    return !is_large(p.paramset) && !p.timeopt && (p.method == M_GINX || p.method == M_LMKCDEY) && p.N == 1024 &&
           p.Q < (1ull << 27) &&
           p.digitsG == 4 && g >= 2 && 4 * g <= 32 && C + p.Q < (1ull << 32) && p.qKS <= 65536 && p.n < 1024;
}

constexpr bool kN2kExtended = true;
bool Engine::n2k_set(const Params& p) {
    // K1w at N = 2048: GINX with digitsG = 4 (q < 2N: the half-resolution table), and under
    // FHE_HIP_N2K_EXT (default on) digitsG 3 / 4 at 29-bit Q and q = 2N (the negated half-range table,
    // digitsG 4 / 5); LMKCDEY with digitsG = 4, and under FHE_HIP_N2K_EXT digitsG 3 (Q < 2^29) and 5
    // (Q < 2^27); the digit fields of d + C in 32 bits
    const uint64_t g = p.gBits, h = 1ull << (g - 1);
    const char* ext = std::getenv("FHE_HIP_N2K_EXT");
    const bool wide_rows = ext ? std::string(ext) == "1" : kN2kExtended;
    // GINX: digitsG 4 at Q < 2^27 (STD256Q); digitsG 3 / 4 at 2^27 <= Q < 2^29 (STD256, STD256_3, STD256_4:
    // the forward transform reduced three times); digitsG 5 at q = 2N (STD256Q_3, STD256Q_4)
    const bool ginx = p.method == M_GINX &&
                      (p.q < 2 * p.N || (p.q == 2 * p.N && (p.Q >= (1ull << 27) || p.digitsG == 5))) &&
                      (p.digitsG == 4 || (p.digitsG == 3 && p.Q >= (1ull << 27) && p.q < 2 * p.N) ||
                       (p.digitsG == 5 && p.q == 2 * p.N && wide_rows));
    // digitsG 3 with 2^27 <= Q < 2^28 (STD256Q_LMKCDEY) measured 24.0K -> 32.7K gates/s
    // (profiles/r04_ext_bench.txt); FHE_HIP_N2K_EXT=0 keeps it on K5
    const bool lmk = p.method == M_LMKCDEY && (p.digitsG == 4 || (wide_rows && (p.digitsG == 3 || p.digitsG == 5)));
    if (lmk && p.Q >= (1ull << 27) && (!wide_rows || p.digitsG == 5)) return false;  // reduced forward: 2-3 digits
    // LMKCDEY: Q < 2^29 (the forward transform reduced once at Q >= 2^27, three times at Q >= 2^28: the
    // 29-bit STD256_3 / STD256_4_LMKCDEY); GINX: Q < 2^27
    const uint64_t qmax = wide_rows ? (1ull << 29) : (1ull << 27);
    if (is_large(p.paramset) || p.timeopt || !(ginx || lmk) || p.N != 2048 || p.Q >= qmax || g < 2 ||
        (uint64_t)p.digitsG * g > 32)
        return false;
    uint64_t C = 0;
    for (uint32_t j = 0; j < p.digitsG; ++j) C += h << (j * g);
    return C + p.Q < (1ull << 32);
}

// The one reader of the kernel knobs: "0" keeps a set off the faster kernel its predicate allows (A/B, tests).
KernelFlags Engine::kernel_flags(const Params& p) {
    auto knob_off = [](const char* name) {
        const char* e = std::getenv(name);
        return e && std::string(e) == "0";
    };
    auto pin = [](const char* name) {  // wave | split | xsplit | qsplit
        const char* e = std::getenv(name);
        const std::string v(e ? e : "");
        return v == "split" ? 2 : v == "wave" ? 1 : v == "xsplit" ? 3 : v == "qsplit" ? 4 : 0;
    };
    KernelFlags f;
    f.wide = !fast_path(p);
    if (!f.wide) {  // the 32-bit path: FHE_HIP_GINX_KERNEL / FHE_HIP_LMK_KERNEL pin its kernel (default by batch size)
        f.ginx_pin = pin("FHE_HIP_GINX_KERNEL");
        f.lmk_pin = pin("FHE_HIP_LMK_KERNEL");
        if (f.lmk_pin == 3) f.lmk_pin = 0;  // LMKCDEY has no xsplit form
        return f;
    }
    f.narrow = narrow_set(p) && !knob_off("FHE_HIP_NARROW");  // "0": keep 64-bit residues
    f.g3 = g3_set(p) && !knob_off("FHE_HIP_GINX3");
    f.n2k = n2k_set(p) && !knob_off("FHE_HIP_N2K");
    if (f.g3) f.ks32 = true;
    else if (ks32_set(p)) f.ks32 = !knob_off("FHE_HIP_KS32");
    else if (ks32w_set(p)) f.ks32w = !knob_off("FHE_HIP_KS32");  // measured +5-15% (profiles/r04_ksw_bench.txt)
    return f;
}

uint32_t Engine::kernel_code(const KernelFlags& f) {
    return !f.wide ? 1 : f.g3 ? 2 : f.n2k ? 4 : f.narrow ? 3 : 0;
}

// The first kernel that serves this launch, fastest first.  The split kernels of the 64-bit path read the u32
// fields of GateArgs (lv, uv, b_const), so they need those equal to the u64 ones; K1m-3 also takes no test-vector
// table (the others say so through their *_supported predicates).
RotationPlan Engine::plan_rotation(const GateArgs& g) const {
    const int nd = (int)p_.digitsG - 1;
    const bool lmk = p_.method == M_LMKCDEY;
    const bool has2 = d_bsk2_ != nullptr;
    const int gw = 2 * (size_t)g.count <= x_batch_ ? 1 : 2;
    if (flags_.wide) {
        const bool same32 = g.lv == g.lv64 && g.uv == g.uv64 && g.b_const == g.b64;
        if (flags_.g3 && lmk && has2 && same32 && !g.tv && !g.tv64)
            return {RotKernel::Lmk3, "k_blind_rotate_lmk3", 0, nd};
        if (flags_.n2k && lmk && has2 && lmk2k_supported(g, tabs2k_, nd) && same32)
            return {RotKernel::Lmk2k, "k_blind_rotate_lmk2k", 0, nd};
        if (lmk || p_.method == M_AP) return {RotKernel::WideOps, "k_blind_rotate_wide_ops", 0, nd};
        if (flags_.n2k && has2 && n2k_supported(g, tabs2k_, nd) && same32)
            return {RotKernel::N2k, "k_blind_rotate_n2k", 0, nd};
        if (flags_.g3 && has2 && ginx3_supported(g, tabs_) && same32)
            return {RotKernel::Ginx3, "k_blind_rotate_ginx2", 0, nd};
        return {RotKernel::Wide, "k_blind_rotate_wide", 0, nd};
    }
    // the kernels' digit decomposition (bootstrap.hip decompose2) works on d + C in 32 bits
    const uint64_t h = 1ull << (g.gbits - 1);
    if (g.gbits < 2 || h * (1 + (1ull << g.gbits) + (1ull << (2 * g.gbits))) + p_.Q >= (1ull << 32))
        throw std::invalid_argument("device path expects log2(baseG) <= 10");
    if (p_.method == M_GINX) {
        // two waves per gate up to x_batch_ gates (K1x: small batches would leave SIMDs idle), K1q (four waves per
        // gate) up to one gate per CU, else one wave per gate; K1x / K1q take gates, BootstrapFunc tables and the
        // seam's accumulators, ciphertext modulus q or 2N
        const int pin = flags_.ginx_pin;
        if (!has2) return {RotKernel::Ginx, "k_blind_rotate_ginx", 0, nd};
        if (pin == 2)
            return ginx2_supported(g, tabs_) ? RotationPlan{RotKernel::Ginx2, "k_blind_rotate_ginx2", 0, nd}
                                             : RotationPlan{RotKernel::Ginx, "k_blind_rotate_ginx", 0, nd};
        if (ginx2x_supported(g, tabs_)) {
            if (pin == 4 || (pin == 0 && 2 * (size_t)g.count <= x_batch_))
                return {RotKernel::Ginx4x, "k_blind_rotate_ginx4x", 0, nd};
            if (pin == 3 || (pin == 0 && g.count <= x_batch_))
                return {RotKernel::Ginx2x, "k_blind_rotate_ginx2x", gw, nd};
        }
        return {RotKernel::Ginx, "k_blind_rotate_ginx", 0, nd};
    }
    // LMKCDEY: four waves per gate up to one gate per CU (K1m-4, as K1q for GINX), two up to x_batch_ gates (one
    // gate per 128-thread workgroup up to one per CU, two per 256-thread workgroup above: k_blind_rotate_lmk3's
    // GW), else the one-wave op-list kernel, which is also AP's
    const int pin = flags_.lmk_pin;
    if (lmk && has2 && pin != 1 && lmkx_supported(g, tabs_)) {
        if (pin == 4 || (pin == 0 && 2 * (size_t)g.count <= x_batch_))
            return {RotKernel::Lmk4x, "k_blind_rotate_lmk4x", 0, nd};
        if (pin == 2 || g.count <= x_batch_) return {RotKernel::LmkX, "k_blind_rotate_lmk3", gw, nd};
    }
    return {RotKernel::Lmk, "k_blind_rotate_lmk", 0, nd};
}

const char* Engine::gate_kernel(size_t count) const {
    return plan_rotation(gate_args(G_AND, count ? count : 1)).name;
}

bool Engine::ks32_set(const Params& p) {
    const bool pow2ks = !(p.qKS & (p.qKS - 1));
    // the tiled shapes (keyswitch.hip launch_keyswitch): baseKS 32 / 64 with digitsKS 3, 16 with 4, and 21 with 4
    // (STD256Q_3, digits by division)
    const bool shape = ((p.baseKS == 32 || p.baseKS == 64) && p.digitsKS == 3) ||
                       ((p.baseKS == 16 || p.baseKS == 21) && p.digitsKS == 4);
    return !is_large(p.paramset) && !p.timeopt && pow2ks && shape && p.qKS <= 65536 && p.n < 2048 && p.N <= 2048;
}

bool Engine::ks32w_set(const Params& p) {
    const bool pow2ks = p.qKS && !(p.qKS & (p.qKS - 1));
    // qKS < 2^32: GateArgs::qKS is a u32 word (launch_keyswitch_w32 reads it from there).  Round 6: also the prime
    // qKS of TOY / SIGNED_MOD_TEST (modKS = PRIME: qKS = Q < 2^28, baseKS 25), whose u32 sums are kept mod qKS
    const bool prime = p.baseKS == 25 && (p.qKS & 1) && p.qKS < (1ull << 28);
    return !is_large(p.paramset) && !p.timeopt && (prime || (pow2ks && p.qKS > 65536 && p.qKS < (1ull << 32))) &&
           keyswitch_w32_shape(p.baseKS, p.digitsKS) && p.n < 2048 && p.N <= 2048;
}

Engine::Engine(int paramset, int method, int device)
    : p_(make_params(paramset, method)), device_(device), flags_(kernel_flags(p_)) {
    // Two accumulator kernels: the 32-bit one (bootstrap.hip) for N = 1024, Q < 2^28, digitsG = 3 (the
    // STD128 / MEDIUM / STD128*_LMKCDEY sets); the 64-bit one (bootstrap_wide.hip) for every other
    // GINX set with N = 1024 / 2048 (any digitsG, Q up to 2^62) and the large-precision family.
    if (flags_.wide) {
        if (p_.N != 512 && p_.N != 1024 && p_.N != 2048)
            throw std::invalid_argument("device path supports ring dimension N = 512 / 1024 / 2048");
        if ((double)p_.digitsG2 * (double)p_.Q >= 18446744073709551616.0)
            throw std::invalid_argument("device path: digitsG2 * Q must stay below 2^64");
        if (p_.q & (p_.q - 1)) throw std::invalid_argument("device path needs a power-of-two q");
        if (p_.n > 2048) throw std::invalid_argument("device path supports n <= 2048");
        FHE_HIP_CHECK(hipSetDevice(device_));
        FHE_HIP_CHECK(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
        build_tables_wide();
        set_base(p_.baseG);
        if (flags_.g3) build_tables();
        if (flags_.n2k) build_tables_n2k();
        if (method == M_LMKCDEY) {  // op lists (k_prep_lmk_w) for k_blind_rotate_wide_ops
            if (p_.n > 2048 || (p_.numAutoKeys + 1) > 0x7fff) throw std::invalid_argument("device path: LMKCDEY n <= 2048");
            build_loggen();
            maxops_ = p_.N + p_.n + 128;
        } else if (method == M_AP) {  // op lists (k_prep_dm_w): at most digitsR ops per index
            if ((size_t)p_.n * p_.baseR * p_.digitsR > 0x8000u) throw std::invalid_argument("device path: AP keys");
            maxops_ = std::max<uint32_t>(p_.N + p_.n + 128, p_.n * p_.digitsR);
        }
        return;
    }
    FHE_HIP_CHECK(hipSetDevice(device_));
    FHE_HIP_CHECK(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    build_tables();
    maxops_ = p_.N + p_.n + 128;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_) == hipSuccess && cus > 0)
        x_batch_ = 2 * (uint32_t)cus;   // K1x: one two-gate workgroup per CU
}

// the DevBuf members free themselves after this: nothing is running by then
Engine::~Engine() {
    (void)hipSetDevice(device_);
    if (stream_) (void)hipStreamSynchronize(stream_);
    if (order_ev_) (void)hipEventDestroy(order_ev_);
    if (stream_) (void)hipStreamDestroy(stream_);
}

hipStream_t Engine::use_stream(hipStream_t s) {
    if (!s) s = stream_;
    if (last_stream_ && s != last_stream_) {  // order after the previous call's work on its stream
        FHE_HIP_CHECK(hipSetDevice(device_));
        // the context's own stream is alive for the context's lifetime: its ordering point is taken
        // now (it covers a synchronous call that threw after enqueueing work); a caller's stream was
        // marked by that call's end_call (capi CallOrder, on every exit path)
        if (last_stream_ == stream_) end_call(stream_);
        if (pending_) FHE_HIP_CHECK(hipStreamWaitEvent(s, order_ev_, 0));
    }
    last_stream_ = s;
    return s;
}

void Engine::end_call(hipStream_t s) {
    FHE_HIP_CHECK(hipSetDevice(device_));
    if (!order_ev_) FHE_HIP_CHECK(hipEventCreateWithFlags(&order_ev_, hipEventDisableTiming));
    FHE_HIP_CHECK(hipEventRecord(order_ev_, s));
    pending_ = true;
}

void Engine::sync_streams() {
    FHE_HIP_CHECK(hipSetDevice(device_));
    FHE_HIP_CHECK(hipStreamSynchronize(stream_));
    if (pending_) FHE_HIP_CHECK(hipEventSynchronize(order_ev_));
}

uint64_t* Engine::reserve(DevBuf& b, size_t bytes) {
    if (bytes <= b.bytes()) return b.as<uint64_t>();
    sync_streams();
    // the call in progress, when it runs on a caller's stream: kernels it has enqueued may read the old block
    if (last_stream_ && last_stream_ != stream_) FHE_HIP_CHECK(hipStreamSynchronize(last_stream_));
    b.alloc(device_, bytes);
    return b.as<uint64_t>();
}

void Engine::set_base(uint32_t bg) {
    cur_ = p_.timeopt ? p_.with_base(bg) : p_;
    cur_off_ = p_.bsk_offset(bg);
    cur_ksk_off_ = p_.ksk_index(bg) * p_.ksk_rows() * ((size_t)p_.n + 1);
}

GateArgs Engine::gate_args(int gate, size_t count, uint32_t p, bool multi) const {
    switch (gate) {
        case G_OR: case G_AND: case G_NOR: case G_NAND: case G_XOR: case G_XNOR: case G_XOR_FAST: case G_XNOR_FAST:
            if (multi) throw std::invalid_argument("EvalBinGate(ctvector): AND3, OR3, AND4, OR4, MAJORITY or CMUX only");
            break;
        case G_MAJORITY: case G_AND3: case G_OR3: case G_AND4: case G_OR4:
            if (!multi) throw std::invalid_argument("EvalBinGate: multi-input gates take a ciphertext vector");
            break;
        default:
            throw std::invalid_argument("EvalBinGate: unsupported gate");
    }
    if (count > 0x7fffffffull) throw std::invalid_argument("batch too large");
    if (p < 2 || 2 * p > p_.q) throw std::invalid_argument("plaintext modulus out of range");
    GateArgs g{};
    g.count = (uint32_t)count;
    g.n = p_.n;
    g.N = p_.N;
    g.q = p_.q;
    g.qKS = p_.qKS;
    g.ctmod = p_.q;
    g.tv = nullptr;
    // BootstrapGateCore window (binfhe-base-scheme.cpp:535-553); Q2p = Q/(2p) + 1 (:555-556)
    const uint64_t q = p_.q, qHalf = q >> 1, Q = p_.Q;
    const uint64_t q1 = p_.gate_const(gate), q2 = (q1 + qHalf) % q;
    const bool swap = q1 >= q2;
    g.lb = (uint32_t)(swap ? q2 : q1);
    g.ub = (uint32_t)(swap ? q1 : q2);
    const uint64_t Q2p = Q / (2 * p) + 1, Q2pNeg = Q - Q2p;
    g.lv = (uint32_t)(swap ? Q2p : Q2pNeg);
    g.uv = (uint32_t)(swap ? Q2pNeg : Q2p);
    g.factor = (uint32_t)(p_.N / qHalf);
    // b = Q/8 + 1 for 2-input gates (:118, hardcoded p = 4), Q/(2p) + 1 for ctvector gates (:162)
    g.b_const = (uint32_t)(multi ? Q / (2 * p) + 1 : (Q >> 3) + 1);
    g.lv64 = swap ? Q2p : Q2pNeg;
    g.uv64 = swap ? Q2pNeg : Q2p;
    g.b64 = multi ? Q / (2 * p) + 1 : (Q >> 3) + 1;
    g.tv64 = nullptr;
    g.xor_double = (gate == G_XOR || gate == G_XNOR || gate == G_XOR_FAST || gate == G_XNOR_FAST) ? 1 : 0;
    g.msb_out = 1;
    g.gbits = p_.gBits;
    return g;
}

// the workspace group grows together: every array to the new count (the first reserve waits, the others find
// the streams idle)
void Engine::ensure_work(size_t count) {
    if (count <= cap_) return;
    cap_ = 0;
    rot_count_ = 0;
    reserve(d_idx_, count * p_.n * sizeof(uint16_t));
    reserve(d_tvb_, count * sizeof(uint32_t));
    if (flags_.wide) {
        reserve(d_wext_a_, count * p_.N * sizeof(uint64_t));
        reserve(d_wext_b_, count * sizeof(uint64_t));
    }
    if (!flags_.wide || flags_.ks32 || flags_.ks32w) {  // ks32 / ks32w: the tiled key switch's u32 input (keyswitch_ext)
        reserve(d_ext_a_, count * p_.N * sizeof(uint32_t));
        reserve(d_ext_b_, count * sizeof(uint32_t));
    }
    if (p_.method == M_LMKCDEY || p_.method == M_AP) {
        reserve(d_ops_, count * maxops_ * sizeof(uint16_t));
        reserve(d_nops_, count * sizeof(uint32_t));
    }
    cap_ = count;
}

void Engine::prep_device(const GateArgs& g, const GateInputs& in, size_t offset, hipStream_t s) {
    if (p_.method == M_GINX) {
        FHE_HIP_CHECK(launch_prep_ginx(g, in, d_idx_ + offset * p_.n, d_tvb_ + offset, s));
    } else if (p_.method == M_AP) {
        if (g.ctmod != p_.q)  // EvalAcc DM reads a_i modulo the parameter q (rgsw-acc-dm.cpp:64-69)
            throw std::invalid_argument("AP accumulator: ciphertext modulus must be q");
        FHE_HIP_CHECK(launch_prep_dm(g, in, d_ops_ + offset * maxops_, d_nops_ + offset, d_tvb_ + offset, maxops_,
                                     p_.baseR, p_.digitsR, s));
    } else {
        FHE_HIP_CHECK(launch_prep_lmk(g, in, d_logGen_, d_ops_ + offset * maxops_,
                                      d_nops_ + offset, d_tvb_ + offset, maxops_, p_.numAutoKeys, s));
    }
}

void Engine::rotate_device(const GateArgs& g, hipStream_t s) {
    rot_count_ = g.count;
    const RotationPlan plan = plan_rotation(g);
    const uint32_t* ek = d_bsk2_.as<const uint32_t>();
    switch (plan.launcher) {
        case RotKernel::Lmk3:
            FHE_HIP_CHECK(launch_blind_rotate_lmk3(g, tabs_, ek, ek + (size_t)p_.n * 12288, d_ops_, d_nops_, maxops_,
                                                   d_tvb_, d_wext_a_, d_wext_b_, s));
            return;
        case RotKernel::Lmk2k: {
            const size_t per = (size_t)2 * 2 * plan.nd * 8 * 64 * 4;  // pack_n2k's ek words per index
            FHE_HIP_CHECK(launch_blind_rotate_lmk2k(g, tabs2k_, ek, ek + (size_t)p_.n * per, d_ops_, d_nops_, maxops_,
                                                    d_tvb_, d_wext_a_, d_wext_b_, plan.nd, s));
            return;
        }
        case RotKernel::N2k:
            FHE_HIP_CHECK(launch_blind_rotate_n2k(g, tabs2k_, d_bsk2_, d_idx_, d_tvb_, d_wext_a_, d_wext_b_, plan.nd, s));
            return;
        case RotKernel::Ginx3:
            FHE_HIP_CHECK(launch_blind_rotate_ginx3(g, tabs_, d_bsk2_, d_idx_, d_tvb_, d_wext_a_, d_wext_b_, s));
            return;
        case RotKernel::WideOps:
        case RotKernel::Wide: {
            WideArgs w{};
            w.count = g.count;
            w.n = g.n;
            w.N = g.N;
            w.ctmod = g.ctmod;
            w.factor = g.factor;
            w.lb = g.lb;
            w.ub = g.ub;
            w.digitsG = cur_.digitsG;
            w.gbits = cur_.gBits;
            w.msb_out = g.msb_out;
            w.lv = g.lv64;
            w.uv = g.uv64;
            w.b_const = g.b64;
            w.qKS = p_.qKS;
            w.tv = g.tv64;
            w.acc_io = g.acc_io;
            w.acc_tv = g.acc_tv;
            w.tv_mod = g.tv_mod;
            if (plan.launcher == RotKernel::Wide) {
                FHE_HIP_CHECK(launch_blind_rotate_wide(w, wtabs_, wkey(cur_off_), d_idx_, d_tvb_, d_wext_a_, d_wext_b_, s));
                return;
            }
            const bool dm = p_.method == M_AP;
            FHE_HIP_CHECK(launch_blind_rotate_wide_ops(w, wtabs_, wkey(0), wkey(dm ? 0 : (size_t)p_.n * p_.digitsG2 * 2 * p_.N),
                                                       d_ops_, d_nops_, maxops_, d_tvb_, d_wext_a_, d_wext_b_, dm, s));
            return;
        }
        case RotKernel::Ginx2:
            FHE_HIP_CHECK(launch_blind_rotate_ginx2(g, tabs_, d_bsk2_, d_idx_, d_tvb_, d_ext_a_, d_ext_b_, s));
            return;
        case RotKernel::Ginx4x:
            FHE_HIP_CHECK(launch_blind_rotate_ginx4x(g, tabs_, d_bsk2_, d_idx_, d_tvb_, d_ext_a_, d_ext_b_, s));
            return;
        case RotKernel::Ginx2x:
            FHE_HIP_CHECK(launch_blind_rotate_ginx2x(g, tabs_, d_bsk2_, d_idx_, d_tvb_, d_ext_a_, d_ext_b_, plan.gw, s));
            return;
        case RotKernel::Ginx:
            FHE_HIP_CHECK(launch_blind_rotate_ginx(g, tabs_, d_bsk_, d_idx_, d_tvb_, d_ext_a_, d_ext_b_, s));
            return;
        case RotKernel::Lmk4x:
            FHE_HIP_CHECK(launch_blind_rotate_lmk4x(g, tabs_, d_bsk2_, p_.n, d_ops_, d_nops_, maxops_, d_tvb_, d_ext_a_,
                                                    d_ext_b_, s));
            return;
        case RotKernel::LmkX:
            FHE_HIP_CHECK(launch_blind_rotate_lmkx(g, tabs_, d_bsk2_, p_.n, d_ops_, d_nops_, maxops_, d_tvb_, d_ext_a_,
                                                   d_ext_b_, plan.gw, s));
            return;
        case RotKernel::Lmk:
            FHE_HIP_CHECK(launch_blind_rotate_lmk(g, tabs_, d_bsk_, d_autok_, d_ops_, d_nops_, maxops_, d_tvb_, d_ext_a_,
                                                  d_ext_b_, p_.method == M_AP, s));
            return;
    }
}

void Engine::bootstrap_device(int gate, size_t count, const uint64_t* a1, const uint64_t* b1, const uint64_t* a2,
                              const uint64_t* b2, bool modswitch, hipStream_t s) {
    if (!d_bsk_) throw std::logic_error("bootstrapping key not loaded");
    GateArgs g = gate_args(gate, count);
    g.msb_out = modswitch ? 1 : 0;
    if (count == 0) return;
    ensure_work(count);
    FHE_HIP_CHECK(hipSetDevice(device_));
    GateInputs in{{a1, a2, nullptr, nullptr}, {b1, b2, nullptr, nullptr}, 2, 0, 0};
    prep_device(g, in, 0, s);
    rotate_device(g, s);
}

void Engine::blind_rotate_acc_device(size_t count, const uint64_t* a, uint32_t ctmod, uint64_t* acc, hipStream_t s) {
    if (!d_bsk_) throw std::logic_error("bootstrapping key not loaded");
    if (ctmod < 2 || (ctmod & (ctmod - 1)) || ctmod > 2 * p_.N)
        throw std::invalid_argument("BlindRotate: ciphertext modulus must be a power of two <= 2N");
    if (p_.method == M_AP && ctmod != p_.q)  // EvalAcc DM reads a_i modulo q (rgsw-acc-dm.cpp:64-69)
        throw std::invalid_argument("BlindRotate (AP): ciphertext modulus must be q");
    if (p_.method == M_LMKCDEY && ctmod != 2 * p_.N)  // a_i are taken mod M = 2N (rgsw-acc-lmkcdey.cpp:84-86)
        throw std::invalid_argument("BlindRotate (LMKCDEY): ciphertext modulus must be 2N");
    if (count == 0) return;
    if (!a || !acc) throw std::invalid_argument("null argument");
    if (count > 0x7fffffffull) throw std::invalid_argument("batch too large");
    ensure_work(count);
    FHE_HIP_CHECK(hipSetDevice(device_));
    GateArgs g{};
    g.count = (uint32_t)count;
    g.n = p_.n;
    g.N = p_.N;
    g.q = p_.q;
    g.qKS = p_.qKS;
    g.ctmod = ctmod;
    g.factor = 2 * p_.N / ctmod;
    g.gbits = p_.gBits;
    g.acc_io = acc;
    // the prep kernels read one input ciphertext; its b only feeds the (unused) test vector
    GateInputs in{{a, nullptr, nullptr, nullptr}, {a, nullptr, nullptr, nullptr}, 1, 0, 0};
    prep_device(g, in, 0, s);
    rotate_device(g, s);
    rot_count_ = 0;  // no ctExt left in the workspace
}

void Engine::blind_rotate_init_device(size_t count, const uint64_t* a, const uint64_t* b, uint64_t* acc, hipStream_t s) {
    if (!d_bsk_) throw std::logic_error("bootstrapping key not loaded");
    if (count == 0) return;
    if (!a || !b || !acc) throw std::invalid_argument("null argument");
    GateArgs g = gate_args(G_AND, count);  // BootstrapGateCore's AND window (Bootstrap, :205)
    ensure_work(count);
    FHE_HIP_CHECK(hipSetDevice(device_));
    g.acc_io = acc;
    g.acc_tv = 1;
    // ct + q/4 (EvalAddConstEq, binfhe-base-scheme.cpp:201): the b offset of the prep
    GateInputs in{{a, nullptr, nullptr, nullptr}, {b, nullptr, nullptr, nullptr}, 1, 0, p_.q >> 2};
    prep_device(g, in, 0, s);
    rotate_device(g, s);
    rot_count_ = 0;
}

void Engine::external_product_device(size_t count, const uint64_t* rgsw, const uint64_t* rlwe, uint64_t* result,
                                     hipStream_t s) {
    if (!flags_.wide && p_.digitsG2 != 4) throw std::invalid_argument("device path expects digitsG = 3");
    if (count == 0) return;
    if (!rgsw || !rlwe || !result) throw std::invalid_argument("null argument");
    FHE_HIP_CHECK(hipSetDevice(device_));
    constexpr size_t kChunk = 0x8000;   // op codes hold key indices < 0x8000
    const size_t keyw = (size_t)p_.digitsG2 * 2 * p_.N;
    const size_t wpk = flags_.wide && !flags_.narrow ? 2 : 1;   // u32 words per packed key word (u64 Montgomery on the 64-bit path)
    const size_t cap = std::min(count, kChunk);
    if (cap > epcap_) {
        epcap_ = 0;
        reserve(d_epk_, cap * keyw * wpk * sizeof(uint32_t));
        reserve(d_epops_, cap * sizeof(uint16_t));
        reserve(d_epn_, cap * sizeof(uint32_t));
        epcap_ = cap;
    }
    const uint32_t ninv_mont = flags_.wide ? 0u : to_mont(invmod(p_.N, p_.Q), p_.Q);
    for (size_t off = 0; off < count; off += kChunk) {
        const size_t c = std::min(kChunk, count - off);
        if (result + off * 2 * p_.N != rlwe + off * 2 * p_.N)
            FHE_HIP_CHECK(hipMemcpyAsync(result + off * 2 * p_.N, rlwe + off * 2 * p_.N, c * 2 * p_.N * 8,
                                         hipMemcpyDeviceToDevice, s));
        FHE_HIP_CHECK(launch_single_ops(d_epops_, d_epn_, (uint32_t)c, 1, s));
        if (flags_.wide) {
            // the wide DM op loop (k_blind_rotate_wide_ops): one EXT op per item with its own key
            FHE_HIP_CHECK(launch_pack_rgsw_wide(rgsw + off * keyw, c * keyw, wtabs_, d_epk_, s));
            WideArgs w{};
            w.count = (uint32_t)c;
            w.n = p_.n;
            w.N = p_.N;
            w.ctmod = p_.q;
            w.factor = 1;
            w.digitsG = p_.digitsG;
            w.gbits = p_.gBits;
            w.qKS = p_.qKS;
            w.acc_io = result + off * 2 * p_.N;
            FHE_HIP_CHECK(launch_blind_rotate_wide_ops(w, wtabs_, d_epk_, d_epk_, d_epops_, d_epn_, 1, nullptr, nullptr,
                                                       nullptr, true, s));
            continue;
        }
        FHE_HIP_CHECK(launch_pack_rgsw(rgsw + off * keyw, c, p_.N, (uint32_t)p_.Q, ninv_mont, d_epk_, s));
        GateArgs g{};
        g.count = (uint32_t)c;
        g.n = p_.n;
        g.N = p_.N;
        g.q = p_.q;
        g.qKS = p_.qKS;
        g.ctmod = p_.q;
        g.factor = 1;
        g.gbits = p_.gBits;
        g.acc_io = result + off * 2 * p_.N;
        // the DM op loop: each item's list is the one external product with its own key
        FHE_HIP_CHECK(launch_blind_rotate_lmk(g, tabs_, d_epk_, nullptr, d_epops_, d_epn_, 1, nullptr, nullptr,
                                              nullptr, true, s));
    }
}

size_t Engine::max_batch() const {
    size_t fr = 0, tot = 0;
    if (hipSetDevice(device_) != hipSuccess || hipMemGetInfo(&fr, &tot) != hipSuccess) return 0;
    // workspace per gate: monomial indices / op list, ctExt, test-vector b, staged I/O
    const size_t per = (size_t)p_.n * 2 + (size_t)maxops_ * 2 + ((size_t)p_.N + 1) * (flags_.wide ? 8 : 4) + 4 +
                       (4 * ((size_t)p_.n + 1) + p_.N + 1) * 8;
    return std::min<size_t>(0x7fffffffull, fr / 2 / per);
}

void Engine::eval_gate_multi_device(int gate, size_t count, uint32_t k, const uint64_t* const* a,
                                    const uint64_t* const* b, uint32_t p, uint64_t* a_out, uint64_t* b_out,
                                    hipStream_t s) {
    if (!ready()) throw std::logic_error("keys not loaded (load_bsk / load_ksk)");
    if (k < 2 || k > 4) throw std::invalid_argument("EvalBinGate(ctvector): 2 to 4 ciphertexts");
    GateArgs g = gate_args(gate, count, p, true);
    if (count == 0) return;
    ensure_work(count);
    FHE_HIP_CHECK(hipSetDevice(device_));
    GateInputs in{};
    for (uint32_t j = 0; j < k; ++j) {
        if (!a[j] || !b[j]) throw std::invalid_argument("null ciphertext array");
        in.a[j] = a[j];
        in.b[j] = b[j];
    }
    in.k = k;
    g.msb_out = a_out ? 1 : 0;
    prep_device(g, in, 0, s);
    rotate_device(g, s);
    if (a_out) keyswitch_workspace_device(count, a_out, b_out, s);
}

void Engine::refresh_device(size_t count, const uint64_t* a, const uint64_t* b, uint64_t* a_out, uint64_t* b_out,
                            hipStream_t s) {
    if (!ready()) throw std::logic_error("keys not loaded (load_bsk / load_ksk)");
    GateArgs g = gate_args(G_AND, count);  // BootstrapGateCore's AND window; b = Q/(2p) + 1, p = 4 (:211)
    if (count == 0) return;
    if (!a || !b || !a_out || !b_out) throw std::invalid_argument("null argument");
    ensure_work(count);
    FHE_HIP_CHECK(hipSetDevice(device_));
    // ct + q/4 (EvalAddConstEq, :201) as the prep's b offset
    GateInputs in{{a, nullptr, nullptr, nullptr}, {b, nullptr, nullptr, nullptr}, 1, 0, p_.q >> 2};
    prep_device(g, in, 0, s);
    rotate_device(g, s);
    keyswitch_workspace_device(count, a_out, b_out, s);
}

void Engine::eval_cmux_device(size_t count, const uint64_t* a0, const uint64_t* b0, const uint64_t* a1,
                              const uint64_t* b1, const uint64_t* a2, const uint64_t* b2, uint64_t* a_out,
                              uint64_t* b_out, hipStream_t s) {
    if (!ready()) throw std::logic_error("keys not loaded (load_bsk / load_ksk)");
    if (count == 0) return;
    if (2 * count > 0x7fffffffull) throw std::invalid_argument("batch too large");
    ensure_work(2 * count);
    FHE_HIP_CHECK(hipSetDevice(device_));
    cmux_levels(count, a0, b0, a1, b1, a2, b2, nullptr, nullptr, a_out, b_out, s);
}

void Engine::cmux_levels(size_t count, const uint64_t* a0, const uint64_t* b0, const uint64_t* a1, const uint64_t* b1,
                         const uint64_t* a2, const uint64_t* b2, const uint64_t* a2n, const uint64_t* b2n,
                         uint64_t* a_out, uint64_t* b_out, hipStream_t s) {
    const size_t n = p_.n;
    uint64_t* l1 = reserve(l1_, 2 * count * (n + 1) * 8);
    uint64_t* l1a = l1;                 // [2 count][n]: NAND(ct0, NOT ct2) | NAND(ct1, ct2)
    uint64_t* l1b = l1 + 2 * count * n; // [2 count]
    const GateArgs gh = gate_args(G_NAND, count);
    // ct0 + NOT ct2: EvalNOT (:223-236) folded into the input combination (ct0 - ct2, b offset q/4; exact
    // mod the power-of-two q), or the explicit NOT column when ct2 was switched from Q
    const GateInputs lo = a2n ? GateInputs{{a0, a2n, nullptr, nullptr}, {b0, b2n, nullptr, nullptr}, 2, 0u, 0u}
                              : GateInputs{{a0, a2, nullptr, nullptr}, {b0, b2, nullptr, nullptr}, 2, 2u, p_.q >> 2};
    const GateInputs hi{{a1, a2, nullptr, nullptr}, {b1, b2, nullptr, nullptr}, 2, 0u, 0u};
    prep_device(gh, lo, 0, s);
    prep_device(gh, hi, count, s);
    rotate_device(gate_args(G_NAND, 2 * count), s);
    keyswitch_workspace_device(2 * count, l1a, l1b, s);
    const GateInputs top{{l1a, l1a + count * n, nullptr, nullptr}, {l1b, l1b + count, nullptr, nullptr}, 2, 0u, 0u};
    prep_device(gh, top, 0, s);
    rotate_device(gh, s);
    keyswitch_workspace_device(count, a_out, b_out, s);
}

void Engine::ext_to_device(size_t count, uint64_t* a_out, uint64_t* b_out, hipStream_t s) {
    if (count > rot_count_) throw std::logic_error("ctExt of more ciphertexts than the last blind rotation produced");
    if (flags_.wide) {
        FHE_HIP_CHECK(hipMemcpyAsync(a_out, d_wext_a_, count * p_.N * 8, hipMemcpyDeviceToDevice, s));
        FHE_HIP_CHECK(hipMemcpyAsync(b_out, d_wext_b_, count * 8, hipMemcpyDeviceToDevice, s));
        return;
    }
    FHE_HIP_CHECK(launch_widen_u64(d_ext_a_, d_ext_b_, a_out, b_out, p_.N, count, s));
}

void Engine::switch_column_device(size_t count, const uint64_t* a, const uint64_t* b, uint32_t stride,
                                  const uint8_t* large, bool negate, bool set_b, uint64_t b_large, uint64_t* a_out,
                                  uint64_t* b_out, hipStream_t s) {
    // ModSwitch(Q -> qKS) into the key switch's input, KeySwitch + ModSwitch(qKS -> q) (K2's epilogue) into
    // the output column, then the rows that were mod q already copied in (lwe-pke.cpp:170-178)
    FHE_HIP_CHECK(launch_switch_in(a, b, stride, large, p_.Q, p_.qKS, p_.N, count, negate,
                                   flags_.wide ? (void*)d_wext_a_ : (void*)d_ext_a_, flags_.wide ? (void*)d_wext_b_ : (void*)d_ext_b_,
                                   flags_.wide, s));
    keyswitch_ext(count, p_.q, a_out, b_out, s);
    FHE_HIP_CHECK(launch_switch_out(a, b, stride, large, p_.n, p_.q, count, negate, set_b, b_large, a_out, b_out, s));
    rot_count_ = 0;  // the workspace no longer holds a blind rotation's ctExt
}

void Engine::switch_to_qn_device(size_t count, const uint64_t* a, const uint64_t* b, uint64_t* a_out, uint64_t* b_out,
                                 hipStream_t s) {
    if (!d_ksk_ && !d_wksk_) throw std::logic_error("key-switching key not loaded");
    if (count == 0) return;
    if (!a || !b || !a_out || !b_out) throw std::invalid_argument("null argument");
    if (count > 0x7fffffffull) throw std::invalid_argument("batch too large");
    ensure_work(count);
    FHE_HIP_CHECK(hipSetDevice(device_));
    switch_column_device(count, a, b, p_.N, nullptr, false, false, 0, a_out, b_out, s);
}

void Engine::eval_mixed_device(int op, uint32_t k, uint32_t ptmod, size_t count, const uint64_t* const* a,
                               const uint64_t* const* b, const uint8_t* const* large, uint64_t* a_out, uint64_t* b_out,
                               bool extended, hipStream_t s) {
    if (!ready()) throw std::logic_error("keys not loaded (load_bsk / load_ksk)");
    const bool multi = op == G_MAJORITY || op == G_AND3 || op == G_OR3 || op == G_AND4 || op == G_OR4;
    if (op == kOpBootstrap) {
        if (k != 1) throw std::invalid_argument("Bootstrap takes one ciphertext");
        if (ptmod < 1) throw std::invalid_argument("plaintext modulus out of range");
    } else if (op == G_CMUX) {
        if (k != 3) throw std::invalid_argument("CMUX gate implemented for ciphertext vectors of size 3");
    } else if (multi) {
        if (k < 2 || k > 4) throw std::invalid_argument("EvalBinGate(ctvector): 2 to 4 ciphertexts");
        gate_args(op, count, ptmod, true);
    } else {
        if (k != 2) throw std::invalid_argument("EvalBinGate: two ciphertexts");
        gate_args(op, count);
    }
    if (count == 0) return;
    if (!a || !b || !a_out || !b_out) throw std::invalid_argument("null argument");
    for (uint32_t j = 0; j < k; ++j)
        if (!a[j] || !b[j]) throw std::invalid_argument("null ciphertext array");
    if ((op == G_CMUX ? 2 : 1) * count > 0x7fffffffull) throw std::invalid_argument("batch too large");
    ensure_work(op == G_CMUX ? 2 * count : count);
    FHE_HIP_CHECK(hipSetDevice(device_));
    const size_t n = p_.n, col = count * (n + 1);
    bool any = false;
    for (uint32_t j = 0; j < k; ++j) any |= large && large[j];
    const bool cmux_not = op == G_CMUX && large && large[2];
    uint64_t* mix = any ? reserve(mix_, (k + (cmux_not ? 1 : 0)) * col * 8) : nullptr;
    // Bootstrap (:199-201): ct + (ct->GetModulus() >> 2) by ModAddFast at the switched ciphertext's modulus q.
    // For an input mod Q that sum is b_sw + Q/4 - q >= 1.5 q, and BootstrapGateCore's window walk
    // (:562-567, ModSubFast by 1 from there) never wraps and never enters [lb, ub < q): every test-vector
    // slot is uv.  The device prep adds q/4 mod q to b; the b its window test then sees, (lb - 1) mod q,
    // walks exactly the complement of [lb, ub), so the same all-uv test vector results.
    const GateArgs gand = gate_args(G_AND, count);
    if (op == kOpBootstrap && any && (p_.Q >> 2) < 2 * (uint64_t)p_.q + (p_.q >> 1))
        throw std::invalid_argument("Bootstrap of a ciphertext mod Q needs Q/4 >= 2.5 q");
    const uint64_t q = p_.q, b_large = ((uint64_t)gand.lb + 2 * q - 1 - (q >> 2)) % q;
    const uint64_t* ia[4] = {};
    const uint64_t* ib[4] = {};
    for (uint32_t j = 0; j < k; ++j) {
        if (large && large[j]) {
            uint64_t* ca = mix + j * col;
            uint64_t* cb = ca + count * n;
            switch_column_device(count, a[j], b[j], p_.N, large[j], false, op == kOpBootstrap, b_large, ca, cb, s);
            ia[j] = ca;
            ib[j] = cb;
        } else {
            ia[j] = a[j];
            ib[j] = b[j];
        }
    }
    if (op == G_CMUX) {
        const uint64_t *a2n = nullptr, *b2n = nullptr;
        if (cmux_not) {  // EvalNOT at ct2's own modulus (:180, :223-236), then the NAND's SwitchCTtoqn
            uint64_t* ca = mix + k * col;
            uint64_t* cb = ca + count * n;
            switch_column_device(count, a[2], b[2], p_.N, large[2], true, false, 0, ca, cb, s);
            a2n = ca;
            b2n = cb;
        }
        cmux_levels(count, ia[0], ib[0], ia[1], ib[1], ia[2], ib[2], a2n, b2n, a_out, b_out, s);
        return;
    }
    if (op == kOpBootstrap) {
        // the window and its values are p = 4's (the switched / copied ciphertext's default plaintext
        // modulus, lwe-ciphertext.h:161); the extraction's b uses the input's own (:210-211)
        GateArgs g = gand;
        g.b_const = (uint32_t)(p_.Q / (2 * (uint64_t)ptmod) + 1);
        g.b64 = p_.Q / (2 * (uint64_t)ptmod) + 1;
        g.msb_out = extended ? 0 : 1;
        const GateInputs in{{ia[0], nullptr, nullptr, nullptr}, {ib[0], nullptr, nullptr, nullptr}, 1, 0, p_.q >> 2};
        prep_device(g, in, 0, s);
        rotate_device(g, s);
    } else if (multi) {
        GateArgs g = gate_args(op, count, ptmod, true);
        g.msb_out = extended ? 0 : 1;
        GateInputs in{};
        for (uint32_t j = 0; j < k; ++j) {
            in.a[j] = ia[j];
            in.b[j] = ib[j];
        }
        in.k = k;
        prep_device(g, in, 0, s);
        rotate_device(g, s);
    } else {
        bootstrap_device(op, count, ia[0], ib[0], ia[1], ib[1], !extended, s);
    }
    if (extended)
        ext_to_device(count, a_out, b_out, s);
    else
        keyswitch_workspace_device(count, a_out, b_out, s);
}

void Engine::keyswitch_workspace_device(size_t count, uint64_t* a_out, uint64_t* b_out, hipStream_t s) {
    if (!d_ksk_ && !d_wksk_) throw std::logic_error("key-switching key not loaded");
    if (count == 0) return;
    if (count > rot_count_)
        throw std::invalid_argument("key switch of more ciphertexts than the last blind rotation produced");
    FHE_HIP_CHECK(hipSetDevice(device_));
    keyswitch_ext(count, p_.q, a_out, b_out, s);
}

void Engine::keyswitch_ext(size_t count, uint64_t q_out, uint64_t* a_out, uint64_t* b_out, hipStream_t s) {
    if (flags_.wide && flags_.ks32 && d_ksk_ && d_ext_a_ && count <= cap_) {
        // the u64 ctExt mod qKS narrowed to u32, then the 32-bit (u16-row, gate-tiled) key switch instead
        // of u64 row gathers
        FHE_HIP_CHECK(launch_narrow_u32(d_wext_a_, d_wext_b_, d_ext_a_, d_ext_b_, p_.N, count, s));
        GateArgs g = gate_args(G_AND, count);
        FHE_HIP_CHECK(launch_keyswitch(g, p_.baseKS, p_.digitsKS, d_ksk_, d_ext_a_, d_ext_b_, q_out, a_out, b_out, s,
                                       ks_part(count), kKsPartWords));
        return;
    }
    if (flags_.wide && flags_.ks32w && d_ksk32_ && d_ext_a_ && count <= cap_) {
        FHE_HIP_CHECK(launch_narrow_u32(d_wext_a_, d_wext_b_, d_ext_a_, d_ext_b_, p_.N, count, s));
        GateArgs g = gate_args(G_AND, count);
        FHE_HIP_CHECK(launch_keyswitch_w32(g, p_.baseKS, p_.digitsKS, d_ksk32_, d_ext_a_, d_ext_b_, q_out, a_out, b_out,
                                           s, ks_part(count), kKsPartWords));
        return;
    }
    if (flags_.wide) {
        const size_t rows = p_.ksk_rows();
        const uint64_t* ksk = d_wksk_ + cur_ksk_off_;  // timeOptimization: the switching key of the current base
        FHE_HIP_CHECK(launch_keyswitch_wide(count, p_.n, p_.N, p_.baseKS, p_.digitsKS, p_.qKS, ksk, ksk + rows * p_.n,
                                            d_wext_a_, d_wext_b_, q_out, a_out, b_out, s));
        return;
    }
    GateArgs g = gate_args(G_AND, count);
    FHE_HIP_CHECK(launch_keyswitch(g, p_.baseKS, p_.digitsKS, d_ksk_, d_ext_a_, d_ext_b_, q_out, a_out, b_out, s,
                                   ks_part(count), kKsPartWords));
}

// scratch of the row-split key switch (launch_keyswitch, below 4096 gates): S count <= 2^16 for
// every count, so 2^16 partial rows of ksk_width / 2 words
uint32_t* Engine::ks_part(size_t count) {
    if (count >= 4096) return nullptr;
    reserve(d_kspart_, kKsPartWords * sizeof(uint32_t));
    return d_kspart_;
}

void Engine::eval_gate_device(int gate, size_t count, const uint64_t* a1, const uint64_t* b1, const uint64_t* a2,
                              const uint64_t* b2, uint64_t* a_out, uint64_t* b_out, hipStream_t s) {
    if (!ready()) throw std::logic_error("keys not loaded (load_bsk / load_ksk)");
    if (count == 0) return;
    bootstrap_device(gate, count, a1, b1, a2, b2, true, s);
    keyswitch_workspace_device(count, a_out, b_out, s);
}

}  // namespace fhe_amd
