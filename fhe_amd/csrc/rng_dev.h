// rng_dev.h -- the counter generator's draws on the device (keygen.h): draw k of a stream whose state is s0.
#pragma once
#include <hip/hip_runtime.h>

#include "keygen.h"

namespace fhe_amd {
namespace {

__device__ __forceinline__ uint64_t draw(uint64_t s0, uint64_t k) { return mix64(s0 + (k + 2) * kRngGamma); }
__device__ __forceinline__ uint64_t draw_uniform(uint64_t s0, uint64_t k, uint64_t m) {
    return __umul64hi(draw(s0, k), m);
}
// the reference's discrete Gaussian (keygen.h dgg_sample) on the host's table, lifted mod m
__device__ __forceinline__ uint64_t draw_dgg(uint64_t s0, uint64_t k, uint64_t m, const DggTable& t) {
    const int64_t v = dgg_sample(draw(s0, k), t);
    return v < 0 ? (uint64_t)(v + (int64_t)m) : (uint64_t)v;
}

}  // namespace
}  // namespace fhe_amd
