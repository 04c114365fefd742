// circuit_engine.cpp -- Engine::eval_circuit_device: a finalized Circuit (circuit.h) evaluated level by level
// on the device.  Per level: indexed prep over the level's slots (bootstrap.hip PoolFetch), the unchanged
// blind rotation with AND's window (rotate_device picks the kernel by the launch's slot count), the unchanged
// key switch straight into the level's block of pool rows.  DESIGN.md §4 "Circuits".
#include <algorithm>
#include <string>

#include "engine.h"

namespace fhe_amd {

void Engine::prep_level_device(const GateArgs& g, const CircuitLevel& lv, hipStream_t s) {
    if (p_.method == M_GINX) {
        FHE_HIP_CHECK(launch_prep_ginx_pool(g, lv, d_idx_, d_tvb_, s));
    } else if (p_.method == M_AP) {
        FHE_HIP_CHECK(launch_prep_dm_pool(g, lv, d_ops_, d_nops_, d_tvb_, maxops_, p_.baseR, p_.digitsR, s));
    } else {
        FHE_HIP_CHECK(launch_prep_lmk_pool(g, lv, d_logGen_, d_ops_, d_nops_, d_tvb_, maxops_, p_.numAutoKeys, s));
    }
}

void Engine::eval_circuit_device(const Circuit& c, size_t B, const uint64_t* a_in, const uint64_t* b_in,
                                 uint64_t* a_out, uint64_t* b_out, hipStream_t s) {
    if (!c.finalized()) throw std::logic_error("circuit is not finalized");
    if (!ready()) throw std::logic_error("keys not loaded (load_bsk / load_ksk)");
    if (B == 0) return;
    const size_t n = p_.n, n_in = c.num_inputs(), n_out = c.num_outputs(), rows = c.num_rows();
    if ((n_in && (!a_in || !b_in)) || (n_out && (!a_out || !b_out))) throw std::invalid_argument("null argument");
    if (B > 0x7fffffffull || rows * B > 0x7fffffffull) throw std::invalid_argument("batch too large");
    FHE_HIP_CHECK(hipSetDevice(device_));

    // widest launch: a whole level, or the chunk limit
    size_t chunk = max_batch();
    if (c.max_slots()) chunk = std::min(chunk, c.max_slots());
    if (chunk == 0) throw AllocError("circuit: no device memory for a launch");
    size_t widest = 0;
    for (size_t l = 1; l <= c.num_levels(); ++l) widest = std::max(widest, c.level_width(l) * B);
    // the pool: every node's B ciphertexts, no row reuse; refused when it would not fit
    const size_t pool_bytes = rows * B * (n + 1) * 8;
    if (pool_bytes > poolcap_) {
        size_t fr = 0, tot = 0;
        FHE_HIP_CHECK(hipMemGetInfo(&fr, &tot));
        if (pool_bytes > fr + poolcap_)
            throw AllocError("circuit: a pool of " + std::to_string(pool_bytes) + " bytes exceeds the device's free memory (" +
                             std::to_string(fr) + " bytes)");
    }
    uint64_t* pool_a = grow(d_pool_, poolcap_, pool_bytes);
    uint64_t* pool_b = pool_a + rows * B * n;
    if (widest) ensure_work(std::min(widest, chunk));

    // descriptors: resident until another circuit is evaluated on this context (a blocking upload, so two
    // evaluations of one circuit queue back to back without touching the host copy)
    const size_t n_slots = c.num_bootstraps();
    const size_t desc_bytes = (n_slots * sizeof(CircuitSlot) + 7) / 8 * 8;
    if (cdesc_serial_ != c.serial()) {
        const std::vector<CircuitSlot> slots = c.slots(p_);
        const std::vector<CircuitOut> outs = c.outputs();
        sync_streams();  // the previous circuit's kernels may still read the old descriptors
        cdesc_serial_ = 0;
        grow(d_cdesc_, cdesccap_, desc_bytes + n_out * sizeof(CircuitOut) + 8);
        if (n_slots)
            FHE_HIP_CHECK(hipMemcpy(d_cdesc_, slots.data(), n_slots * sizeof(CircuitSlot), hipMemcpyHostToDevice));
        if (n_out)
            FHE_HIP_CHECK(hipMemcpy(reinterpret_cast<char*>(d_cdesc_) + desc_bytes, outs.data(),
                                    n_out * sizeof(CircuitOut), hipMemcpyHostToDevice));
        cdesc_serial_ = c.serial();
    }
    const CircuitSlot* d_slots = reinterpret_cast<const CircuitSlot*>(d_cdesc_);
    const CircuitOut* d_outs = reinterpret_cast<const CircuitOut*>(reinterpret_cast<const char*>(d_cdesc_) + desc_bytes);

    // inputs are the pool's first rows: input j, instance i at row j B + i, the caller's layout
    if (n_in) {
        FHE_HIP_CHECK(hipMemcpyAsync(pool_a, a_in, n_in * B * n * 8, hipMemcpyDeviceToDevice, s));
        FHE_HIP_CHECK(hipMemcpyAsync(pool_b, b_in, n_in * B * 8, hipMemcpyDeviceToDevice, s));
    }
    for (size_t l = 1; l <= c.num_levels(); ++l) {
        const size_t row0 = c.level_row(l), width = c.level_width(l), total = width * B;
        for (size_t first = 0; first < total; first += chunk) {
            const size_t cnt = std::min(chunk, total - first);
            const GateArgs g = gate_args(G_AND, cnt);
            const CircuitLevel lv{pool_a, pool_b, d_slots + (row0 - n_in), (uint32_t)width, (uint32_t)B, (uint32_t)first};
            prep_level_device(g, lv, s);
            rotate_device(g, s);
            keyswitch_ext(cnt, p_.q, pool_a + (row0 * B + first) * n, pool_b + row0 * B + first, s);
        }
    }
    if (n_out)
        FHE_HIP_CHECK(launch_circuit_gather(pool_a, pool_b, d_outs, (uint32_t)n_out, (uint32_t)B, p_.n, p_.q, a_out, b_out, s));
}

void Engine::eval_circuit_host(const Circuit& c, size_t B, const uint64_t* a_in, const uint64_t* b_in, uint64_t* a_out,
                               uint64_t* b_out) {
    if (!c.finalized()) throw std::logic_error("circuit is not finalized");
    if (B == 0) return;
    const size_t n = p_.n, n_in = c.num_inputs(), n_out = c.num_outputs();
    if ((n_in && (!a_in || !b_in)) || (n_out && (!a_out || !b_out))) throw std::invalid_argument("null argument");
    if (B > 0x7fffffffull || c.num_rows() * B > 0x7fffffffull) throw std::invalid_argument("batch too large");
    FHE_HIP_CHECK(hipSetDevice(device_));
    uint64_t* d = grow(d_cio_, ciocap_, (n_in + n_out) * B * (n + 1) * 8 + 8);
    uint64_t* dai = d;
    uint64_t* dbi = dai + n_in * B * n;
    uint64_t* dao = dbi + n_in * B;
    uint64_t* dbo = dao + n_out * B * n;
    if (n_in) {
        FHE_HIP_CHECK(hipMemcpyAsync(dai, a_in, n_in * B * n * 8, hipMemcpyHostToDevice, stream_));
        FHE_HIP_CHECK(hipMemcpyAsync(dbi, b_in, n_in * B * 8, hipMemcpyHostToDevice, stream_));
    }
    eval_circuit_device(c, B, dai, dbi, dao, dbo, stream_);
    if (n_out) {
        FHE_HIP_CHECK(hipMemcpyAsync(a_out, dao, n_out * B * n * 8, hipMemcpyDeviceToHost, stream_));
        FHE_HIP_CHECK(hipMemcpyAsync(b_out, dbo, n_out * B * 8, hipMemcpyDeviceToHost, stream_));
    }
    FHE_HIP_CHECK(hipStreamSynchronize(stream_));
}

}  // namespace fhe_amd
