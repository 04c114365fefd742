// pke_engine.cpp -- Engine's public-key entry points: the resident public key (load_pubkey / pubkeygen_device)
// and EncryptN batches (encrypt_pk_device) on the kernels of pke.hip; SMALL_DIM output is the existing
// SwitchCTtoqn prelude (switch_to_qn_device) on the kernel's dimension-N ciphertexts.  DESIGN.md §4 "Public-key
// encryption".
#include <algorithm>
#include <utility>
#include <vector>

#include "engine.h"
#include "keygen.h"
#include "pke.h"

namespace fhe_amd {

void Engine::load_pubkey(const uint64_t* A, const uint64_t* v) {
    if (!A || !v) throw std::invalid_argument("null argument");
    const size_t N = p_.N;
    const uint64_t Q = p_.Q;
    for (size_t k = 0; k < N * N; ++k)
        if (A[k] >= Q) throw std::invalid_argument("public key not reduced mod Q");
    for (size_t j = 0; j < N; ++j)
        if (v[j] >= Q) throw std::invalid_argument("public key not reduced mod Q");
    FHE_HIP_CHECK(hipSetDevice(device_));
    sync_streams();
    d_pk_.release();
    DevArr<void> key;  // becomes the resident key once it is whole
    key.alloc(device_, pk_key_bytes(p_.N, Q));
    uint64_t* dv = key.as<uint64_t>();
    FHE_HIP_CHECK(hipMemcpy(dv, v, N * 8, hipMemcpyHostToDevice));
    if (pk_word32(Q)) {
        std::vector<uint32_t> a32(N * N);
        for (size_t k = 0; k < N * N; ++k) a32[k] = (uint32_t)A[k];
        FHE_HIP_CHECK(hipMemcpy(dv + N, a32.data(), N * N * 4, hipMemcpyHostToDevice));
    } else {
        FHE_HIP_CHECK(hipMemcpy(dv + N, A, N * N * 8, hipMemcpyHostToDevice));
    }
    d_pk_ = std::move(key);
}

void Engine::pubkeygen_device(const uint64_t* skN, size_t N, uint64_t seed, uint64_t* A_out, uint64_t* v_out) {
    if (!skN) throw std::invalid_argument("ring secret is null");
    if (N != p_.N) throw std::invalid_argument("ring secret has wrong length");
    std::vector<int32_t> s;
    ring_secret_signed(p_, skN, s);
    FHE_HIP_CHECK(hipSetDevice(device_));
    sync_streams();
    d_pk_.release();
    DevArr<void> key;  // becomes the resident key once it is whole
    DevBuf ds, raw;    // the signed secret and, when the caller asked for A, its u64 copy
    try {
        key.alloc(device_, pk_key_bytes(p_.N, p_.Q));
        ds.alloc(device_, N * sizeof(int32_t));
        if (A_out) raw.alloc(device_, N * N * 8);
        FHE_HIP_CHECK(hipMemcpyAsync(ds.as<>(), s.data(), N * sizeof(int32_t), hipMemcpyHostToDevice, stream_));
        FHE_HIP_CHECK(launch_pk_gen(seed, p_.N, p_.Q, ds.as<const int32_t>(), key, raw.as<uint64_t>(), stream_));
        if (A_out) FHE_HIP_CHECK(hipMemcpyAsync(A_out, raw.as<>(), N * N * 8, hipMemcpyDeviceToHost, stream_));
        if (v_out) FHE_HIP_CHECK(hipMemcpyAsync(v_out, key, N * 8, hipMemcpyDeviceToHost, stream_));
        FHE_HIP_CHECK(hipStreamSynchronize(stream_));  // the temporaries are freed on return
    } catch (...) {
        (void)hipStreamSynchronize(stream_);
        throw;
    }
    d_pk_ = std::move(key);
}

void Engine::encrypt_pk_device(const int32_t* d_bits, size_t count, uint64_t first, uint64_t seed, uint32_t ptmod,
                               int output, uint64_t* a_out, uint64_t* b_out, hipStream_t s) {
    if (ptmod < 2 || ptmod > p_.Q) throw std::invalid_argument("plaintext modulus out of range");
    if (output != kLargeDim && output != kSmallDim) throw std::invalid_argument("output: LARGE_DIM (3) or SMALL_DIM (4)");
    if (!d_pk_) throw std::logic_error("public key not loaded (load_pubkey / pubkeygen_device)");
    if (output == kSmallDim && !d_ksk_ && !d_wksk_) throw std::logic_error("key-switching key not loaded");
    if (count == 0) return;
    if (!d_bits || !a_out || !b_out) throw std::invalid_argument("null argument");
    if (count > 0x7fffffffull) throw std::invalid_argument("batch too large");
    const size_t N = p_.N, spw = (pk_sp_words(p_.N, count) + 1) / 2;
    const bool small = output == kSmallDim;
    uint64_t* w = reserve(pkw_, (spw + (small ? count * (N + 1) : 0)) * 8);
    if (small) ensure_work(count);  // before anything is enqueued: growing the workspace synchronises
    FHE_HIP_CHECK(hipSetDevice(device_));
    uint64_t* la = small ? w + spw : a_out;
    uint64_t* lb = small ? la + count * N : b_out;
    FHE_HIP_CHECK(launch_encrypt_pk(seed, first, p_.N, p_.Q, ptmod, d_pk_, d_bits, count,
                                    reinterpret_cast<uint32_t*>(w), la, lb, s));
    if (small) switch_to_qn_device(count, la, lb, a_out, b_out, s);
}

}  // namespace fhe_amd
