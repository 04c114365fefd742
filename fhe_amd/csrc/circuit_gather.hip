// circuit_gather.hip -- output gather of a circuit evaluation (Engine::eval_circuit_device): the requested pool
// rows into the caller's dense [n_out][B][n] / [n_out][B] arrays.  A streaming copy, one thread per word.
#include "boot.h"

#include <algorithm>

namespace fhe_amd {

namespace {
__global__ void k_circuit_gather(const uint64_t* __restrict__ pa, const uint64_t* __restrict__ pb,
                                 const CircuitOut* __restrict__ outs, uint32_t n_out, uint32_t B, uint32_t n, uint64_t q,
                                 uint64_t* __restrict__ ao, uint64_t* __restrict__ bo) {
    const uint64_t rows = (uint64_t)n_out * B, total = rows * n;
    for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; t < total; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t r = t / n, i = t - r * n, o = r / B, inst = r - o * B;
        const CircuitOut d = outs[o];
        const uint64_t x = pa[((uint64_t)d.src * B + inst) * n + i];
        ao[t] = d.neg ? (x ? q - x : 0) : x;  // EvalNOT: a = -a mod q
    }
    for (uint64_t r = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; r < rows; r += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t o = r / B, inst = r - o * B;
        const CircuitOut d = outs[o];
        const uint64_t x = pb[(uint64_t)d.src * B + inst];
        bo[r] = d.neg ? ((q >> 2) + q - x) % q : x;  // b = q/4 - b mod q
    }
}
}  // namespace

hipError_t launch_circuit_gather(const uint64_t* pool_a, const uint64_t* pool_b, const CircuitOut* outs, uint32_t n_out,
                                 uint32_t B, uint32_t n, uint32_t q, uint64_t* a_out, uint64_t* b_out, hipStream_t s) {
    if (n_out == 0 || B == 0) return hipSuccess;
    if (!pool_a || !pool_b || !outs || !a_out || !b_out || n == 0 || q == 0) return hipErrorInvalidValue;
    const uint64_t total = (uint64_t)n_out * B * n;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((total + 255) / 256, 4096);
    hipLaunchKernelGGL(k_circuit_gather, dim3(blocks), dim3(256), 0, s, pool_a, pool_b, outs, n_out, B, n, (uint64_t)q,
                       a_out, b_out);
    return hipGetLastError();
}

}  // namespace fhe_amd
