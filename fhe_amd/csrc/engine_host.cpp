// engine_host.cpp -- Engine's synchronous host-buffer entry points.  Each one lists its staged arrays once
// (host_call: a Carver sizes the staging block and hands the sub-arrays out in the listed order), uploads them, runs
// the _device entry point on the context's stream, copies the outputs back and synchronises.  See engine.h.
#include <algorithm>
#include <vector>

#include "circuit.h"
#include "engine.h"
#include "pke.h"

namespace fhe_amd {

void Engine::copy_ext_host(size_t count, uint64_t* ext_a, uint64_t* ext_b) {
    const size_t N = p_.N;
    if (flags_.wide) {
        FHE_HIP_CHECK(hipMemcpyAsync(ext_a, d_wext_a_, count * N * 8, hipMemcpyDeviceToHost, stream_));
        FHE_HIP_CHECK(hipMemcpyAsync(ext_b, d_wext_b_, count * 8, hipMemcpyDeviceToHost, stream_));
        FHE_HIP_CHECK(hipStreamSynchronize(stream_));
        return;
    }
    std::vector<uint32_t> ha(count * N), hb(count);
    FHE_HIP_CHECK(hipMemcpyAsync(ha.data(), d_ext_a_, count * N * 4, hipMemcpyDeviceToHost, stream_));
    FHE_HIP_CHECK(hipMemcpyAsync(hb.data(), d_ext_b_, count * 4, hipMemcpyDeviceToHost, stream_));
    FHE_HIP_CHECK(hipStreamSynchronize(stream_));
    for (size_t i = 0; i < count * N; ++i) ext_a[i] = ha[i];
    for (size_t i = 0; i < count; ++i) ext_b[i] = hb[i];
}

template <typename Run>
void Engine::host_call(const std::vector<HostIn>& in, size_t aw, size_t bw, uint64_t* a_out, uint64_t* b_out, Run&& run) {
    Carver cv;
    for (const HostIn& x : in) cv.add(x.words);
    cv.add(aw);
    cv.add(bw);
    cv.bind(reserve(stage_, cv.words() * 8));
    FHE_HIP_CHECK(hipSetDevice(device_));
    std::vector<uint64_t*> d;
    for (const HostIn& x : in) {
        d.push_back(cv.take(x.words));
        if (x.src && x.bytes) FHE_HIP_CHECK(hipMemcpyAsync(d.back(), x.src, x.bytes, hipMemcpyHostToDevice, stream_));
    }
    uint64_t* dao = cv.take(aw);
    uint64_t* dbo = cv.take(bw);
    run(d.data(), dao, dbo);
    if (aw) FHE_HIP_CHECK(hipMemcpyAsync(a_out, dao, aw * 8, hipMemcpyDeviceToHost, stream_));
    if (bw) FHE_HIP_CHECK(hipMemcpyAsync(b_out, dbo, bw * 8, hipMemcpyDeviceToHost, stream_));
    FHE_HIP_CHECK(hipStreamSynchronize(stream_));
}

// run(da, db, dao, dbo): da[j] / db[j] the staged column j.  staged_out false: the call leaves ctExt in the
// workspace and the caller collects it (copy_ext_host); dao / dbo are then null.
template <typename Run>
void Engine::host_columns(size_t count, uint32_t k, const uint64_t* const* a, const uint64_t* const* b, bool staged_out,
                          uint64_t* a_out, uint64_t* b_out, Run&& run) {
    const size_t n = p_.n;
    std::vector<HostIn> in;
    for (uint32_t j = 0; j < k; ++j) {
        in.push_back({a[j], count * n, count * n * 8});
        in.push_back({b[j], count, count * 8});
    }
    host_call(in, staged_out ? count * n : 0, staged_out ? count : 0, a_out, b_out,
              [&](uint64_t* const* d, uint64_t* dao, uint64_t* dbo) {
                  const uint64_t* da[4] = {};
                  const uint64_t* db[4] = {};
                  for (uint32_t j = 0; j < k; ++j) {
                      da[j] = d[2 * j];
                      db[j] = d[2 * j + 1];
                  }
                  run(da, db, staged_out ? dao : nullptr, staged_out ? dbo : nullptr);
              });
}

void Engine::eval_gate_host(int gate, size_t count, const uint64_t* a1, const uint64_t* b1, const uint64_t* a2,
                            const uint64_t* b2, uint64_t* a_out, uint64_t* b_out) {
    if (count == 0) return;
    const uint64_t* a[2] = {a1, a2};
    const uint64_t* b[2] = {b1, b2};
    host_columns(count, 2, a, b, true, a_out, b_out,
                 [&](const uint64_t* const* da, const uint64_t* const* db, uint64_t* dao, uint64_t* dbo) {
                     eval_gate_device(gate, count, da[0], db[0], da[1], db[1], dao, dbo, stream_);
                 });
}

void Engine::bootstrap_extended_host(int gate, size_t count, const uint64_t* a1, const uint64_t* b1,
                                     const uint64_t* a2, const uint64_t* b2, uint64_t* ext_a, uint64_t* ext_b) {
    if (count == 0) return;
    const uint64_t* a[2] = {a1, a2};
    const uint64_t* b[2] = {b1, b2};
    host_columns(count, 2, a, b, false, nullptr, nullptr,
                 [&](const uint64_t* const* da, const uint64_t* const* db, uint64_t*, uint64_t*) {
                     bootstrap_device(gate, count, da[0], db[0], da[1], db[1], false, stream_);
                 });
    copy_ext_host(count, ext_a, ext_b);
}

void Engine::keyswitch_host(size_t count, const uint64_t* a, const uint64_t* b, uint64_t* a_out, uint64_t* b_out) {
    if (!d_ksk_ && !d_wksk_) throw std::logic_error("key-switching key not loaded");
    if (count == 0) return;
    ensure_work(count);
    const size_t N = p_.N, n = p_.n;
    for (size_t i = 0; i < count * N; ++i)
        if (a[i] >= p_.qKS) throw std::invalid_argument("keyswitch input not reduced mod qKS");
    for (size_t i = 0; i < count; ++i)
        if (b[i] >= p_.qKS) throw std::invalid_argument("keyswitch input not reduced mod qKS");
    // the input goes straight into the workspace's ctExt (u32 words on the 32-bit path), not through the staging
    std::vector<uint32_t> ha, hb;
    if (!flags_.wide) {
        ha.assign(a, a + count * N);
        hb.assign(b, b + count);
    }
    host_call({}, count * n, count, a_out, b_out, [&](uint64_t* const*, uint64_t* dao, uint64_t* dbo) {
        if (flags_.wide) {
            FHE_HIP_CHECK(hipMemcpyAsync(d_wext_a_, a, count * N * 8, hipMemcpyHostToDevice, stream_));
            FHE_HIP_CHECK(hipMemcpyAsync(d_wext_b_, b, count * 8, hipMemcpyHostToDevice, stream_));
        } else {
            FHE_HIP_CHECK(hipMemcpyAsync(d_ext_a_, ha.data(), count * N * 4, hipMemcpyHostToDevice, stream_));
            FHE_HIP_CHECK(hipMemcpyAsync(d_ext_b_, hb.data(), count * 4, hipMemcpyHostToDevice, stream_));
        }
        keyswitch_ext(count, 0, dao, dbo, stream_);
    });
}

void Engine::eval_gate_multi_host(int gate, size_t count, uint32_t k, const uint64_t* const* a,
                                  const uint64_t* const* b, uint32_t p, uint64_t* a_out, uint64_t* b_out,
                                  bool extended) {
    if (k < 2 || k > 4) throw std::invalid_argument("EvalBinGate(ctvector): 2 to 4 ciphertexts");
    gate_args(gate, count, p, true);  // validate before any transfer
    if (count == 0) return;
    for (uint32_t j = 0; j < k; ++j)
        if (!a[j] || !b[j]) throw std::invalid_argument("null ciphertext array");
    host_columns(count, k, a, b, !extended, a_out, b_out,
                 [&](const uint64_t* const* da, const uint64_t* const* db, uint64_t* dao, uint64_t* dbo) {
                     eval_gate_multi_device(gate, count, k, da, db, p, dao, dbo, stream_);
                 });
    if (extended) copy_ext_host(count, a_out, b_out);
}

void Engine::refresh_host(size_t count, const uint64_t* a, const uint64_t* b, uint64_t* a_out, uint64_t* b_out) {
    if (count == 0) return;
    if (!a || !b) throw std::invalid_argument("null ciphertext array");
    host_columns(count, 1, &a, &b, true, a_out, b_out,
                 [&](const uint64_t* const* da, const uint64_t* const* db, uint64_t* dao, uint64_t* dbo) {
                     refresh_device(count, da[0], db[0], dao, dbo, stream_);
                 });
}

void Engine::eval_cmux_host(size_t count, const uint64_t* a0, const uint64_t* b0, const uint64_t* a1,
                            const uint64_t* b1, const uint64_t* a2, const uint64_t* b2, uint64_t* a_out,
                            uint64_t* b_out) {
    if (count == 0) return;
    const uint64_t* a[3] = {a0, a1, a2};
    const uint64_t* b[3] = {b0, b1, b2};
    for (uint32_t j = 0; j < 3; ++j)
        if (!a[j] || !b[j]) throw std::invalid_argument("null ciphertext array");
    host_columns(count, 3, a, b, true, a_out, b_out,
                 [&](const uint64_t* const* da, const uint64_t* const* db, uint64_t* dao, uint64_t* dbo) {
                     eval_cmux_device(count, da[0], db[0], da[1], db[1], da[2], db[2], dao, dbo, stream_);
                 });
}

void Engine::eval_mixed_host(int op, uint32_t k, uint32_t ptmod, size_t count, const uint64_t* const* a,
                             const uint64_t* const* b, const uint8_t* const* large, uint64_t* a_out, uint64_t* b_out,
                             bool extended) {
    if (k < 1 || k > 4) throw std::invalid_argument("1 to 4 ciphertext columns");
    if (count == 0) return;
    const size_t n = p_.n, N = p_.N;
    // staged columns (rows of N words where flagged) each with its flags (count bytes), and the output
    std::vector<HostIn> in;
    for (uint32_t j = 0; j < k; ++j) {
        if (!a[j] || !b[j]) throw std::invalid_argument("null ciphertext array");
        const bool lg = large && large[j];
        const size_t len = lg ? N : n;
        in.push_back({a[j], count * len, count * len * 8});
        in.push_back({b[j], count, count * 8});
        in.push_back({lg ? large[j] : nullptr, (count + 7) / 8, count});
    }
    const size_t outlen = extended && op != G_CMUX ? N : n;
    host_call(in, count * outlen, count, a_out, b_out, [&](uint64_t* const* d, uint64_t* dao, uint64_t* dbo) {
        const uint64_t* da[4] = {};
        const uint64_t* db[4] = {};
        const uint8_t* dl[4] = {};
        for (uint32_t j = 0; j < k; ++j) {
            da[j] = d[3 * j];
            db[j] = d[3 * j + 1];
            if (large && large[j]) dl[j] = reinterpret_cast<const uint8_t*>(d[3 * j + 2]);
        }
        eval_mixed_device(op, k, ptmod, count, da, db, dl, dao, dbo, extended, stream_);
    });
}

void Engine::switch_to_qn_host(size_t count, const uint64_t* a, const uint64_t* b, uint64_t* a_out, uint64_t* b_out) {
    if (count == 0) return;
    const size_t n = p_.n, N = p_.N;
    host_call({{a, count * N, count * N * 8}, {b, count, count * 8}}, count * n, count, a_out, b_out,
              [&](uint64_t* const* d, uint64_t* dao, uint64_t* dbo) {
                  switch_to_qn_device(count, d[0], d[1], dao, dbo, stream_);
              });
}

void Engine::eval_circuit_host(const Circuit& c, size_t B, const uint64_t* a_in, const uint64_t* b_in, uint64_t* a_out,
                               uint64_t* b_out) {
    if (!c.finalized()) throw std::logic_error("circuit is not finalized");
    if (B == 0) return;
    const size_t n = p_.n, n_in = c.num_inputs(), n_out = c.num_outputs();
    if ((n_in && (!a_in || !b_in)) || (n_out && (!a_out || !b_out))) throw std::invalid_argument("null argument");
    if (B > 0x7fffffffull || c.num_rows() * B > 0x7fffffffull) throw std::invalid_argument("batch too large");
    // the trailing word keeps the block non-empty for a circuit without inputs and outputs
    host_call({{a_in, n_in * B * n, n_in * B * n * 8}, {b_in, n_in * B, n_in * B * 8}, {nullptr, 1, 0}}, n_out * B * n,
              n_out * B, a_out, b_out, [&](uint64_t* const* d, uint64_t* dao, uint64_t* dbo) {
                  eval_circuit_device(c, B, d[0], d[1], dao, dbo, stream_);
              });
}

// op: 0 func, 1 floor, 2 sign, 3 decomp, 4 bootstrap_func, 5 multi-output EvalFunc (engine.h)
void Engine::fb_host(int op, size_t count, const uint64_t* a, const uint64_t* b, uint64_t arg, uint64_t arg2,
                     uint32_t iarg, const uint64_t* lut, uint64_t* a_out, uint64_t* b_out) {
    if (!ready()) throw std::logic_error("keys not loaded (load_bsk / load_ksk)");
    if (count == 0) return;
    const size_t n = p_.n;
    const size_t parts = op == 3 ? eval_decomp_parts(arg) : op == 5 ? iarg : 1;
    host_call({{a, count * n, count * n * 8}, {b, count, count * 8}}, parts * count * n, parts * count, a_out, b_out,
              [&](uint64_t* const* d, uint64_t* oa, uint64_t* ob) {
                  const uint64_t *da = d[0], *db = d[1];
                  switch (op) {
                      case 0: eval_func_device(count, da, db, arg, lut, oa, ob, stream_); break;
                      case 1: eval_floor_device(count, da, db, arg, iarg, oa, ob, stream_); break;
                      case 2: eval_sign_device(count, da, db, arg, iarg != 0, oa, ob, stream_); break;
                      case 3: eval_decomp_device(count, da, db, arg, oa, ob, stream_); break;
                      case 4: bootstrap_func_device(count, da, db, (uint32_t)arg, lut, arg2, oa, ob, stream_); break;
                      case 5: eval_func_multi_device(count, da, db, arg, lut, iarg, oa, ob, stream_); break;
                      default: throw std::invalid_argument("unknown functional-bootstrapping op");
                  }
              });
}

void Engine::encrypt_pk_host(const int* bits, size_t count, uint64_t first, uint64_t seed, uint32_t ptmod, int output,
                             uint64_t* a_out, uint64_t* b_out) {
    if (count == 0 || (output != kLargeDim && output != kSmallDim)) {  // the refusals, or nothing to do
        encrypt_pk_device(nullptr, 0, first, seed, ptmod, output, nullptr, nullptr, stream_);
        return;
    }
    if (!bits || !a_out || !b_out) throw std::invalid_argument("null argument");
    if (count > 0x7fffffffull) throw std::invalid_argument("batch too large");
    const size_t len = output == kSmallDim ? p_.n : p_.N;
    host_call({{bits, (count + 1) / 2, count * sizeof(int32_t)}}, count * len, count, a_out, b_out,
              [&](uint64_t* const* d, uint64_t* da, uint64_t* db) {
                  encrypt_pk_device(reinterpret_cast<const int32_t*>(d[0]), count, first, seed, ptmod, output, da, db,
                                    stream_);
              });
}

}  // namespace fhe_amd
