// circuit_engine.cpp -- Engine::eval_circuit_device: a finalized Circuit (circuit.h) evaluated level by level
// on the device.  Per level and launch class (gates in AND's window, tables at q, tables at 2q, multi-input gates
// per plaintext modulus other than 4): indexed prep
// over the class's slots (bootstrap.hip PoolFetch), the unchanged blind rotation (rotate_device picks the kernel
// by the launch's slot count), the unchanged key switch straight into the class's block of pool rows; then the
// level's LINEAR rows in one element-wise launch.  DESIGN.md §4 "Circuits".
#include <algorithm>
#include <string>

#include "engine.h"

namespace fhe_amd {

void Engine::prep_level_device(const GateArgs& g, const CircuitLevel& lv, hipStream_t s) {
    if (p_.method == M_GINX) {
        FHE_HIP_CHECK(launch_prep_ginx_pool(g, lv, d_idx_, d_tvb_, s));
    } else if (p_.method == M_AP) {
        if (g.ctmod != p_.q)  // EvalAcc DM reads a_i modulo the parameter q (rgsw-acc-dm.cpp:64-69)
            throw std::invalid_argument("AP accumulator: ciphertext modulus must be q");
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
    // FUNC nodes against this parameter set (LUT length, the arbitrary class): refused before anything is touched
    c.check_params(p_);
    const size_t nt1 = c.num_tables(1), nt2 = c.num_tables(2);
    const uint32_t cm1 = Circuit::table_ctmod(p_, 1), cm2 = Circuit::table_ctmod(p_, 2);
    if ((nt1 && cm1 > 2 * p_.N) || (nt2 && cm2 > 2 * p_.N))
        throw std::invalid_argument("ctmod must be a power of two <= 2N");
    FHE_HIP_CHECK(hipSetDevice(device_));

    // widest launch: a whole class of a level, or the chunk limit
    size_t chunk = max_batch();
    if (c.max_slots()) chunk = std::min(chunk, c.max_slots());
    if (chunk == 0) throw AllocError("circuit: no device memory for a launch");
    size_t widest = 0;
    for (size_t l = 1; l <= c.num_levels(); ++l) {
        size_t w[4];
        c.level_classes(l, w);
        widest = std::max(widest, std::max(w[0], std::max(w[1], w[2])) * B);
        for (const auto& gc : c.level_gate_classes(l)) widest = std::max(widest, gc.second * B);
    }
    // the pool: every node's B ciphertexts, no row reuse; refused when it would not fit
    const size_t pool_bytes = rows * B * (n + 1) * 8;
    if (pool_bytes > pool_.bytes()) {
        size_t fr = 0, tot = 0;
        FHE_HIP_CHECK(hipMemGetInfo(&fr, &tot));
        if (pool_bytes > fr + pool_.bytes())
            throw AllocError("circuit: a pool of " + std::to_string(pool_bytes) + " bytes exceeds the device's free memory (" +
                             std::to_string(fr) + " bytes)");
    }
    uint64_t* pool_a = reserve(pool_, pool_bytes);
    uint64_t* pool_b = pool_a + rows * B * n;
    if (widest) ensure_work(std::min(widest, chunk));

    // descriptors and tables: resident until another circuit is evaluated on this context (a blocking upload, so
    // two evaluations of one circuit queue back to back without touching the host copy).  Layout, each part
    // rounded up to 8 bytes: slots, outputs, LINEAR rows, class-1 tables, class-2 tables (u32 words, u64 on the
    // wide path, already scaled by Q / fmod).
    auto up8 = [](size_t x) { return (x + 7) / 8 * 8; };
    const size_t n_slots = c.num_bootstraps(), n_lin = c.num_linears(), tw = flags_.wide ? 8 : 4;
    const size_t desc_bytes = up8(n_slots * sizeof(CircuitSlot));
    const size_t lin_off = desc_bytes + up8(n_out * sizeof(CircuitOut));
    const size_t tab_off[3] = {0, lin_off + up8(n_lin * sizeof(CircuitLinear)),
                               lin_off + up8(n_lin * sizeof(CircuitLinear)) + up8(nt1 * cm1 * tw)};
    const size_t all_bytes = tab_off[2] + up8(nt2 * cm2 * tw) + 8;
    if (cdesc_serial_ != c.serial()) {
        const std::vector<CircuitSlot> slots = c.slots(p_);
        const std::vector<CircuitOut> outs = c.outputs();
        const std::vector<CircuitLinear> lins = c.linears(p_);
        sync_streams();  // the previous circuit's kernels may still read the old descriptors
        cdesc_serial_ = 0;
        char* base = reinterpret_cast<char*>(reserve(cdesc_, all_bytes));
        if (n_slots) FHE_HIP_CHECK(hipMemcpy(base, slots.data(), n_slots * sizeof(CircuitSlot), hipMemcpyHostToDevice));
        if (n_out)
            FHE_HIP_CHECK(hipMemcpy(base + desc_bytes, outs.data(), n_out * sizeof(CircuitOut), hipMemcpyHostToDevice));
        if (n_lin) FHE_HIP_CHECK(hipMemcpy(base + lin_off, lins.data(), n_lin * sizeof(CircuitLinear), hipMemcpyHostToDevice));
        for (int cls = 1; cls <= 2; ++cls) {
            if (!c.num_tables(cls)) continue;
            const std::vector<uint64_t> tv = c.tables(p_, cls);
            if (flags_.wide) {
                FHE_HIP_CHECK(hipMemcpy(base + tab_off[cls], tv.data(), tv.size() * 8, hipMemcpyHostToDevice));
            } else {
                const std::vector<uint32_t> tv32(tv.begin(), tv.end());
                FHE_HIP_CHECK(hipMemcpy(base + tab_off[cls], tv32.data(), tv32.size() * 4, hipMemcpyHostToDevice));
            }
        }
        cdesc_serial_ = c.serial();
    }
    const char* dbase = cdesc_.as<const char>();
    const CircuitSlot* d_slots = reinterpret_cast<const CircuitSlot*>(dbase);
    const CircuitOut* d_outs = reinterpret_cast<const CircuitOut*>(dbase + desc_bytes);
    const CircuitLinear* d_lins = reinterpret_cast<const CircuitLinear*>(dbase + lin_off);

    // the launch's arguments per class: AND's window, the class's tables as bootstrap_func_tables builds them, or
    // (cls 3) AND's window with lv / uv / b_const from Q/(2 ptmod) + 1 -- which is what gate_args builds for
    // MAJORITY at that modulus, q1(MAJORITY) being q1(AND)
    auto class_args = [&](int cls, size_t cnt, uint32_t ptmod) {
        if (cls == 0) return gate_args(G_AND, cnt);
        if (cls == 3) return gate_args(G_MAJORITY, cnt, ptmod, true);
        GateArgs g{};
        g.count = (uint32_t)cnt;
        g.n = p_.n;
        g.N = p_.N;
        g.q = p_.q;
        g.qKS = p_.qKS;
        g.ctmod = cls == 1 ? cm1 : cm2;
        g.factor = 2 * p_.N / g.ctmod;
        g.tv = flags_.wide ? nullptr : reinterpret_cast<const uint32_t*>(dbase + tab_off[cls]);
        g.tv64 = flags_.wide ? reinterpret_cast<const uint64_t*>(dbase + tab_off[cls]) : nullptr;
        g.tv_mod = 0;   // the table comes per slot, in the high half of tvb
        g.b_const = 0;  // ctExt = (acc0, acc1[0]) (binfhe-base-scheme.cpp:624-626)
        g.msb_out = 1;
        g.gbits = p_.gBits;
        return g;
    };
    auto linear_level = [&](size_t l) {
        size_t w[4];
        c.level_classes(l, w);
        if (!w[3]) return;
        const size_t row0 = c.level_row(l) + c.level_width(l) - w[3];
        FHE_HIP_CHECK(launch_circuit_linear(pool_a, pool_b, d_lins + c.level_linear(l), (uint32_t)w[3], (uint32_t)B, p_.n, p_.q,
                                            (uint32_t)row0, s));
    };

    // inputs are the pool's first rows: input j, instance i at row j B + i, the caller's layout
    if (n_in) {
        FHE_HIP_CHECK(hipMemcpyAsync(pool_a, a_in, n_in * B * n * 8, hipMemcpyDeviceToDevice, s));
        FHE_HIP_CHECK(hipMemcpyAsync(pool_b, b_in, n_in * B * 8, hipMemcpyDeviceToDevice, s));
    }
    linear_level(0);
    for (size_t l = 1; l <= c.num_levels(); ++l) {
        size_t w[4];
        c.level_classes(l, w);
        size_t row0 = c.level_row(l), slot0 = c.level_slot(l);
        const auto& gcs = c.level_gate_classes(l);
        for (size_t ci = 0; ci < 3 + gcs.size(); ++ci) {  // the level's classes in row order
            const int cls = ci < 3 ? (int)ci : 3;
            const uint32_t ptmod = ci < 3 ? 0 : gcs[ci - 3].first;
            const size_t width = ci < 3 ? w[ci] : gcs[ci - 3].second, total = width * B;
            if (!width) continue;
            const uint64_t fmod = cls == 2 ? cm2 : p_.q;  // every stage's output modulus is its ciphertext modulus
            for (size_t first = 0; first < total; first += chunk) {
                const size_t cnt = std::min(chunk, total - first);
                const GateArgs g = class_args(cls, cnt, ptmod);
                const CircuitLevel lv{pool_a, pool_b, d_slots + slot0, (uint32_t)width, (uint32_t)B, (uint32_t)first};
                prep_level_device(g, lv, s);
                rotate_device(g, s);
                keyswitch_ext(cnt, fmod, pool_a + (row0 * B + first) * n, pool_b + row0 * B + first, s);
            }
            if (cls == 2) {  // SetModulus(q) of the second stages' outputs (:305), in place: the rows users see are mod q
                const size_t s1 = c.level_arb_stage1(l), r2 = (row0 + s1) * B, cnt2 = (width - s1) * B;
                if (cnt2)
                    FHE_HIP_CHECK(launch_lwe_reduce(pool_a + r2 * n, pool_b + r2, pool_a + r2 * n, pool_b + r2, p_.q, (uint32_t)n,
                                                    cnt2, s));
            }
            row0 += width;
            slot0 += width;
        }
        linear_level(l);
    }
    if (n_out)
        FHE_HIP_CHECK(launch_circuit_gather(pool_a, pool_b, d_outs, (uint32_t)n_out, (uint32_t)B, p_.n, p_.q, a_out, b_out, s));
}

}  // namespace fhe_amd
