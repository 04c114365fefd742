// pke.h -- launchers of the public-key kernels (pke.hip): PubKeyGen and EncryptN on the device.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "keygen.h"

namespace fhe_amd {

// k_encrypt_pk's tile: a workgroup owns kPkTileG ciphertexts (one thread each) x kPkTileC columns of a, and
// stages kPkTileR rows of that column slice of A in LDS at a time
constexpr uint32_t kPkTileG = 128;
constexpr uint32_t kPkTileC = 16;
constexpr uint32_t kPkTileR = 32;

// the resident public key: v [N] u64, then A [N][N] row-major in u32 words when Q < 2^31, else u64
inline bool pk_word32(uint64_t Q) { return Q < (1ull << 31); }
inline size_t pk_key_bytes(uint32_t N, uint64_t Q) { return (size_t)N * 8 + (size_t)N * N * (pk_word32(Q) ? 4 : 8); }
// words of the packed ternary draws of `count` ciphertexts: [N / 16][count] u32, 2 bits per s'_j
inline size_t pk_sp_words(uint32_t N, size_t count) { return (size_t)(N / 16) * count; }

// PubKeyGen (lwe-pke.cpp:74-98) into the resident layout at d_key; s [N]: the signed secret; raw_A (may be
// null) receives A as u64 words
hipError_t launch_pk_gen(uint64_t seed, uint32_t N, uint64_t Q, const int32_t* d_s, void* d_key, uint64_t* raw_A,
                         hipStream_t s);
// EncryptN (lwe-pke.cpp:133-167) of ciphertexts [first, first + count) of stream seed: messages d_bits [count],
// d_sp scratch of pk_sp_words(N, count) words; a_out [count][N], b_out [count] mod Q
hipError_t launch_encrypt_pk(uint64_t seed, uint64_t first, uint32_t N, uint64_t Q, uint32_t ptmod, const void* d_key,
                             const int32_t* d_bits, size_t count, uint32_t* d_sp, uint64_t* a_out, uint64_t* b_out,
                             hipStream_t s);

}  // namespace fhe_amd
