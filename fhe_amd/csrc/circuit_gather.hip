// circuit_gather.hip -- output gather of a circuit evaluation (Engine::eval_circuit_device): the requested pool
// rows into the caller's dense [n_out][B][n] / [n_out][B] arrays, a streaming copy, one thread per word; and the
// LINEAR rows of a level (k_circuit_linear), an element-wise signed sum of up to four pool rows.
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
// LINEAR rows of one level: row row0 + node, instance inst = sum of up to four signed source rows, + c on b, mod q
// (a power of two).  Word w of a ciphertext's n + 1 is a[w], the last one b; consecutive threads take
// consecutive words.  The sources lie in earlier rows than any row written here (a LINEAR operand is never LINEAR).
__global__ void k_circuit_linear(uint64_t* __restrict__ pa, uint64_t* __restrict__ pb, const CircuitLinear* __restrict__ desc,
                                 uint32_t nodes, uint32_t B, uint32_t n, uint32_t row0, uint64_t qm) {
    const uint64_t total = (uint64_t)nodes * B * (n + 1);
    for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; t < total; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t r = t / (n + 1), w = t - r * (n + 1), node = r / B, inst = r - node * B;
        const CircuitLinear d = desc[node];
        uint64_t s = w == n ? d.c : 0;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            if (j < d.k) {
                const uint64_t src = (uint64_t)d.src[j] * B + inst;
                const uint64_t x = w == n ? pb[src] : pa[src * n + w];
                s += ((d.neg_mask >> j) & 1) ? 0 - x : x;
            }
        }
        const uint64_t dst = ((uint64_t)row0 + node) * B + inst;
        if (w == n) pb[dst] = s & qm;
        else pa[dst * n + w] = s & qm;
    }
}
}  // namespace

hipError_t launch_circuit_linear(uint64_t* pool_a, uint64_t* pool_b, const CircuitLinear* desc, uint32_t nodes, uint32_t B,
                                 uint32_t n, uint32_t q, uint32_t row0, hipStream_t s) {
    if (nodes == 0 || B == 0) return hipSuccess;
    if (!pool_a || !pool_b || !desc || n == 0 || q == 0 || (q & (q - 1))) return hipErrorInvalidValue;
    const uint64_t total = (uint64_t)nodes * B * (n + 1);
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((total + 255) / 256, 4096);
    hipLaunchKernelGGL(k_circuit_linear, dim3(blocks), dim3(256), 0, s, pool_a, pool_b, desc, nodes, B, n, row0,
                       (uint64_t)q - 1);
    return hipGetLastError();
}

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
