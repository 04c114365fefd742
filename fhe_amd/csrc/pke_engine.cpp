// pke_engine.cpp -- Engine's public-key entry points: the resident public key (load_pubkey / pubkeygen_device)
// and EncryptN batches (encrypt_pk_device) on the kernels of pke.hip; SMALL_DIM output is the existing
// SwitchCTtoqn prelude (switch_to_qn_device) on the kernel's dimension-N ciphertexts.  DESIGN.md §4 "Public-key
// encryption".
#include <algorithm>
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
    if (d_pk_) FHE_HIP_CHECK(hipFree(d_pk_));
    d_pk_ = nullptr;
    void* key = nullptr;
    FHE_HIP_CHECK(hipMalloc(&key, pk_key_bytes(p_.N, Q)));
    try {
        uint64_t* dv = static_cast<uint64_t*>(key);
        FHE_HIP_CHECK(hipMemcpy(dv, v, N * 8, hipMemcpyHostToDevice));
        if (pk_word32(Q)) {
            std::vector<uint32_t> a32(N * N);
            for (size_t k = 0; k < N * N; ++k) a32[k] = (uint32_t)A[k];
            FHE_HIP_CHECK(hipMemcpy(dv + N, a32.data(), N * N * 4, hipMemcpyHostToDevice));
        } else {
            FHE_HIP_CHECK(hipMemcpy(dv + N, A, N * N * 8, hipMemcpyHostToDevice));
        }
    } catch (...) {
        (void)hipFree(key);
        throw;
    }
    d_pk_ = key;
}

void Engine::pubkeygen_device(const uint64_t* skN, size_t N, uint64_t seed, uint64_t* A_out, uint64_t* v_out) {
    if (!skN) throw std::invalid_argument("ring secret is null");
    if (N != p_.N) throw std::invalid_argument("ring secret has wrong length");
    std::vector<int32_t> s;
    ring_secret_signed(p_, skN, s);
    FHE_HIP_CHECK(hipSetDevice(device_));
    sync_streams();
    if (d_pk_) FHE_HIP_CHECK(hipFree(d_pk_));
    d_pk_ = nullptr;
    void *key = nullptr, *ds = nullptr, *raw = nullptr;
    try {
        FHE_HIP_CHECK(hipMalloc(&key, pk_key_bytes(p_.N, p_.Q)));
        FHE_HIP_CHECK(hipMalloc(&ds, N * sizeof(int32_t)));
        if (A_out) FHE_HIP_CHECK(hipMalloc(&raw, N * N * 8));
        FHE_HIP_CHECK(hipMemcpyAsync(ds, s.data(), N * sizeof(int32_t), hipMemcpyHostToDevice, stream_));
        FHE_HIP_CHECK(launch_pk_gen(seed, p_.N, p_.Q, static_cast<const int32_t*>(ds), key,
                                    static_cast<uint64_t*>(raw), stream_));
        if (A_out) FHE_HIP_CHECK(hipMemcpyAsync(A_out, raw, N * N * 8, hipMemcpyDeviceToHost, stream_));
        if (v_out) FHE_HIP_CHECK(hipMemcpyAsync(v_out, key, N * 8, hipMemcpyDeviceToHost, stream_));
        FHE_HIP_CHECK(hipStreamSynchronize(stream_));  // temporaries are freed on return
    } catch (...) {
        (void)hipStreamSynchronize(stream_);
        for (void* ptr : {key, ds, raw})
            if (ptr) (void)hipFree(ptr);
        throw;
    }
    FHE_HIP_CHECK(hipFree(ds));
    if (raw) FHE_HIP_CHECK(hipFree(raw));
    d_pk_ = key;
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
    uint64_t* w = grow(d_pkw_, pkcap_, (spw + (small ? count * (N + 1) : 0)) * 8);
    if (small) ensure_work(count);  // before anything is enqueued: growing the workspace synchronises
    FHE_HIP_CHECK(hipSetDevice(device_));
    uint64_t* la = small ? w + spw : a_out;
    uint64_t* lb = small ? la + count * N : b_out;
    FHE_HIP_CHECK(launch_encrypt_pk(seed, first, p_.N, p_.Q, ptmod, d_pk_, d_bits, count,
                                    reinterpret_cast<uint32_t*>(w), la, lb, s));
    if (small) switch_to_qn_device(count, la, lb, a_out, b_out, s);
}

void Engine::encrypt_pk_host(const int* bits, size_t count, uint64_t first, uint64_t seed, uint32_t ptmod, int output,
                             uint64_t* a_out, uint64_t* b_out) {
    if (count == 0 || (output != kLargeDim && output != kSmallDim)) {  // the refusals, or nothing to do
        encrypt_pk_device(nullptr, 0, first, seed, ptmod, output, nullptr, nullptr, stream_);
        return;
    }
    if (!bits || !a_out || !b_out) throw std::invalid_argument("null argument");
    if (count > 0x7fffffffull) throw std::invalid_argument("batch too large");
    const size_t len = output == kSmallDim ? p_.n : p_.N, bw = (count + 1) / 2;
    uint64_t* d = grow(d_pkio_, pkiocap_, (bw + count * (len + 1)) * 8);
    FHE_HIP_CHECK(hipSetDevice(device_));
    uint64_t* da = d + bw;
    uint64_t* db = da + count * len;
    FHE_HIP_CHECK(hipMemcpyAsync(d, bits, count * sizeof(int32_t), hipMemcpyHostToDevice, stream_));
    encrypt_pk_device(reinterpret_cast<const int32_t*>(d), count, first, seed, ptmod, output, da, db, stream_);
    FHE_HIP_CHECK(hipMemcpyAsync(a_out, da, count * len * 8, hipMemcpyDeviceToHost, stream_));
    FHE_HIP_CHECK(hipMemcpyAsync(b_out, db, count * 8, hipMemcpyDeviceToHost, stream_));
    FHE_HIP_CHECK(hipStreamSynchronize(stream_));
}

}  // namespace fhe_amd
