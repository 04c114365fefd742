/*
 * fhe_hip.h -- C-ABI of the fhe_amd MI355X (gfx950) TFHE bootstrapping engine.
 *
 * Drop-in boundary for the reference's binfhe GPU-backend seam
 * lux::fhe::backend::Backend (src/binfhe/include/backend/backend.h:73-247 in
 * luxcpp/fhe) and for the gate path BinFHEContext::EvalBinGate
 * (src/binfhe/lib/binfhecontext.cpp:309-317) / EvalBinGateBatch
 * (src/binfhe/lib/batch/batch.cpp:176-210).  Plain pointers and sizes only.
 *
 * Conventions (mirroring the reference C API, include/lux/fhe/c_api.h:57-70):
 *   - every entry point returns 0 (FHE_HIP_OK) or a negative FHE_HIP_ERR_*;
 *     no C++ exception ever crosses this boundary (c_api.cpp:224-235);
 *   - the caller owns host buffers; a context owns its device copies;
 *   - host-buffer calls are synchronous; *_device calls are asynchronous on the
 *     given HIP stream (NULL = the context's own stream).  A context has one
 *     device workspace: a call on a different stream than the context's previous
 *     asynchronous call first waits for that call's work (an event recorded on its
 *     stream), so the calls on one context always execute in issue order;
 *   - a context is bound to one device and is not thread-safe: use one per
 *     host thread / device (BinFHEContext is likewise used per process).
 * Integers are the reference's u64 words (NativeInteger, NATIVEINT=64).
 */
#ifndef FHE_HIP_H
#define FHE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* error codes: same meanings as LuxFheError (c_api.h:57-70), plus device errors */
enum {
    FHE_HIP_OK = 0,
    FHE_HIP_ERR_NULL_PTR = -1,
    FHE_HIP_ERR_INVALID_PARAM = -2,
    FHE_HIP_ERR_ALLOC = -3,
    FHE_HIP_ERR_BOOTSTRAP = -7,
    FHE_HIP_ERR_GATE = -8,
    FHE_HIP_ERR_NOT_INIT = -11,
    FHE_HIP_ERR_DEVICE = -20
};

/* ------------------------------------------------------------------------ */
/* Batched negacyclic NTT (NativePoly::SwitchFormat,                         */
/*   src/core/include/lattice/hal/default/poly-impl.h:420-440;               */
/*   transformnat-impl.h:302-373 forward, :511-624 inverse).                 */
/* ------------------------------------------------------------------------ */
typedef struct fhe_hip_ntt_plan fhe_hip_ntt_plan;

/* N a power of two, 4 <= N <= 65536; Q prime, Q = 1 mod 2N, Q < 2^62; anything else
 * is FHE_HIP_ERR_INVALID_PARAM, and fhe_hip_last_error() says which.  psi = 0 picks the
 * reference's root (minimal primitive 2N-th root, nbtheory-impl.h:183-228);
 * *psi_out (optional) receives the root used.  N = 1024 runs the one-polynomial-per-wave
 * kernels; every other N the LDS stage kernels: one pass up to fhe_hip_ntt_onepass_max(),
 * two passes above. */
int fhe_hip_ntt_plan_create(uint64_t Q, uint64_t psi, uint32_t N, int device, fhe_hip_ntt_plan** out,
                            uint64_t* psi_out);
void fhe_hip_ntt_plan_destroy(fhe_hip_ntt_plan* plan);
/* in-place on host memory: polys[count][N], canonical inputs (< Q).
 * inverse = 0: COEFFICIENT -> EVALUATION (bit-reversed); 1: back. */
int fhe_hip_ntt_batch(fhe_hip_ntt_plan* plan, uint64_t* polys, size_t count, int inverse);
/* device memory, asynchronous on `stream` (hipStream_t; NULL = plan stream);
 * d_in may equal d_out. */
int fhe_hip_ntt_batch_device(fhe_hip_ntt_plan* plan, const uint64_t* d_in, uint64_t* d_out, size_t count,
                             int inverse, void* stream);
/* the plan's stream (hipStream_t) */
void* fhe_hip_ntt_plan_stream(fhe_hip_ntt_plan* plan);
/* the plan's ring dimension (0 for a NULL plan) */
uint32_t fhe_hip_ntt_plan_n(fhe_hip_ntt_plan* plan);
/* Negacyclic product out = a b mod (X^N + 1, Q) of count polynomial pairs: two forward
 * transforms, a pointwise product, one inverse (the reference's SwitchFormat / Times /
 * SwitchFormat).  a, b and out are in COEFFICIENT form, canonical words; out may be a or b.
 * The host call is synchronous (count < 2^31).  The device call is asynchronous on `stream`
 * (NULL = plan stream) and keeps the transform of b in a buffer the plan owns: calls on one
 * plan go to one stream, or the caller orders them. */
int fhe_hip_poly_mul_batch(fhe_hip_ntt_plan* plan, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t count);
int fhe_hip_poly_mul_batch_device(fhe_hip_ntt_plan* plan, const uint64_t* d_a, const uint64_t* d_b, uint64_t* d_out,
                                  size_t count, void* stream);
/* How a plan is dispatched.  fhe_hip_ntt_onepass_max: the largest N (N != 1024) transformed in one
 * pass with the polynomial in LDS, per arithmetic width (wide = Q >= 2^30); larger N take two passes.
 * fhe_hip_ntt_plan_dispatch: the plan's passes (1 or 2) and the polynomials one workgroup
 * transforms.
 * Measurement hook, not part of the stable interface: fhe_hip_ntt_plan_set_onepass_max moves one
 * plan's cut (a power of two in 2048 .. 16384; results do not change) so that tools/ntt_sizes_time.py
 * can run both sides of it.  The cut is read on the host when a call enqueues its launches, so work
 * already enqueued is unaffected and only later calls change; like every call on a plan it is not
 * thread-safe. */
uint32_t fhe_hip_ntt_onepass_max(int wide);
int fhe_hip_ntt_plan_dispatch(fhe_hip_ntt_plan* plan, uint32_t* passes, uint32_t* polys_per_group);
int fhe_hip_ntt_plan_set_onepass_max(fhe_hip_ntt_plan* plan, uint32_t n);

/* ------------------------------------------------------------------------ */
/* Gate bootstrapping context (one per device).                             */
/*   Replaces BinFHEContext::EvalBinGate / EvalBinGateBatch and the seam's   */
/*   BlindRotateBatch + KeySwitchBatch + ModSwitchBatch (backend.h:177-211). */
/* Parameter sets / methods / gates use the reference's enum values         */
/*   (src/binfhe/include/binfhe-constants.h:49-126):                         */
/*   paramset TOY=0, STD128=3, STD128_LMKCDEY=21; method GINX=2, LMKCDEY=3;   */
/*   gate OR=0 AND=1 NOR=2 NAND=3 XOR=4 XNOR=5 MAJORITY=6 AND3=7 OR3=8       */
/*   AND4=9 OR4=10 XOR_FAST=11 XNOR_FAST=12 CMUX=13.                        */
/* Raw key layouts (u64 words, the reference's values):                     */
/*   GINX bsk    [n][2 (s=+1, s=-1)][digitsG2][2][N]  EVAL (bit-reversed)   */
/*               = (*BSkey)[0][0..1][i] (rgsw-acc-cggi.cpp:39-57)           */
/*   LMKCDEY bsk [n][digitsG2][2][N] ++ [numAutoKeys+1][digitsG-1][2][N]    */
/*               = (*BSkey)[0][0][i] ++ (*BSkey)[0][1][k] (rgsw-acc-lmkcdey.cpp:39-68) */
/*   ksk A [N][baseKS][digitsKS][n], ksk B [N][baseKS][digitsKS]            */
/*               = LWESwitchingKeyImpl::GetElementsA/B (lwe-keyswitchkey.h:49) */
/* Ciphertexts: a[count][len], b[count] (len n for gate inputs/outputs).    */
/* ------------------------------------------------------------------------ */
typedef struct fhe_hip_ctx fhe_hip_ctx;

typedef struct {
    uint32_t paramset, method, n, N, q, baseKS, digitsKS, baseG, digitsG, numAutoKeys, keyDist;
    uint32_t kernel;  /* the accumulator kernels the set runs on: 1 = 32-bit, one wave per gate (N = 1024,
                         Q < 2^28, digitsG = 3); 2 = 32-bit split, two waves per gate (digitsG = 4, N = 1024,
                         Q < 2^27); 3 = the one-gate-per-workgroup accumulator with 32-bit residues
                         (Q < 2^30, digitsG2 Q < 2^32: the N = 2048 STD256 / STD256Q rows, TOY, ...);
                         4 = GINX gates at N = 2048, Q < 2^27, digitsG = 4, q < 2N (STD256Q) with the
                         accumulator in registers, two waves per gate (the rest as 3);
                         0 = the same accumulator with 64-bit residues (every other set, the
                         large-precision family) */
    uint64_t Q, psi, qKS, bsk_words, ksk_rows;  /* ksk_rows: of the raw layout (timeOptimization: 3 keys) */
} fhe_hip_params;
/* The large-precision family GenerateBinFHEContext(set, arbFunc, logQ, N, GINX, false)
 * (binfhecontext.cpp:55-104: Q = LastPrime(54, 2N), N = 2048, qKS = 2^35, n = 1305 (TOY: 32),
 * baseG 2^14 / 2^18 / 2^27 by logQ) is addressed by the paramset code
 *   FHE_HIP_LARGE | set << 16 | arbFunc << 15 | FHE_HIP_TIMEOPT? | log2(N) << 8 (0: minimum N) | logQ
 * in every entry point that takes a paramset.  FHE_HIP_TIMEOPT is timeOptimization = true: for
 * logQ != 11 the bootstrapping key is BTKeyGen's map (binfhecontext.cpp:285-307), one key per baseG
 * 2^14, 2^18, 2^27 concatenated in that order in the raw bsk (bsk_words covers the three), and
 * EvalSign / EvalDecomp switch keys as the modulus shrinks (binfhe-base-scheme.cpp:409-431, 498-514);
 * gates and the other operations use the key of the set's own baseG. */
#define FHE_HIP_LARGE (1 << 30)
#define FHE_HIP_TIMEOPT (1 << 14)

/* parameters of a set (host only; GenerateBinFHEContext, binfhecontext.cpp:107-179) */
int fhe_hip_params_get(int paramset, int method, fhe_hip_params* out);
int fhe_hip_create(int paramset, int method, int device, fhe_hip_ctx** out);
void fhe_hip_destroy(fhe_hip_ctx* ctx);
/* the context's parameters; its kernel field reports the kernels THIS context runs (the FHE_HIP_* kernel
 * settings it was created under), fhe_hip_params_get's the default for the set */
int fhe_hip_get_params(const fhe_hip_ctx* ctx, fhe_hip_params* out);
/* the blind-rotation kernel a 2-input gate batch of `count` ciphertexts runs on in this context (a static
 * string, e.g. "k_blind_rotate_ginx" / "k_blind_rotate_ginx2x": the rocprof kernel name) */
int fhe_hip_gate_kernel(const fhe_hip_ctx* ctx, size_t count, const char** name);
/* the context's stream (hipStream_t) */
void* fhe_hip_stream(fhe_hip_ctx* ctx);
/* upload keys (BTKeyLoad, binfhecontext.h:273-275; Backend::PackBootstrappingKey) */
int fhe_hip_load_bsk(fhe_hip_ctx* ctx, const uint64_t* bsk, size_t n_words);
int fhe_hip_load_ksk(fhe_hip_ctx* ctx, const uint64_t* A, size_t nA, const uint64_t* B, size_t nB);
/* The resident keys of src (same parameter set and method, any device) into dst: device-to-device copies of
 * the packed key buffers (xGMI peer copies between GPUs), no host repacking -- the per-device key fan-out of
 * fhe_hip_multi_load_keys; a resident public key (fhe_hip_load_pubkey / fhe_hip_pubkeygen_device) is copied too */
int fhe_hip_copy_keys(fhe_hip_ctx* dst, const fhe_hip_ctx* src);
/* BTKeyGen on the context's device (BinFHEContext::BTKeyGen binfhecontext.cpp:185-200 -> KeyGenAcc
 * rgsw-acc-cggi.cpp:39-96 / rgsw-acc-dm.cpp:39-114 / rgsw-acc-lmkcdey.cpp:39-226, KeySwitchGen
 * lwe-pke.cpp:264-344): generates and loads the keys for sk[n] (mod qKS); bit-identical to
 * fhe_hip_keygen(..., seed, ...) for the sk it returns.  Every parameter set, the large-precision family and
 * its timeOptimization map included, is generated on the device straight into the resident layouts: no key is
 * built on the host.  bsk / kskA / kskB (raw layouts, may be NULL) receive a host copy (with
 * timeOptimization the three keys concatenated, the sizes fhe_hip_load_bsk / fhe_hip_load_ksk expect).  On
 * failure the context holds no keys. */
int fhe_hip_btkeygen_device(fhe_hip_ctx* ctx, const uint64_t* sk, size_t n, uint64_t seed, uint64_t* bsk,
                            uint64_t* kskA, uint64_t* kskB);
/* What fhe_hip_btkeygen_device does for a set (host only, no device needed), from the descriptor builder the
 * device generator itself uses: on_device 1 when the set is generated on the device (every supported set);
 * keys 1, or 3 with timeOptimization; row_pairs the RGSW row pairs drawn over all keys (bsk_words / 2N, less
 * AP's never-drawn j = 0 slots); ntt_polys the polynomials handed to the batched NTT (2 per row pair);
 * ksk_rows = N baseKS digitsKS keys; scratch_bytes the peak device memory of the generator's temporaries
 * (descriptors, secrets, one chunk of row pairs capped at 768 MiB, the switching key's vectors; the export
 * buffer of a requested raw bsk and the NTT plan's tables are not counted). */
typedef struct {
    uint32_t on_device, keys;
    uint64_t row_pairs, ntt_polys, ksk_rows, scratch_bytes;
} fhe_hip_keygen_plan;
int fhe_hip_keygen_plan_get(int paramset, int method, fhe_hip_keygen_plan* out);
/* ---- the reference's packed transfer format (src/binfhe/include/backend/packed.h:29-307) ----
 * LWE batches byte-compatible with PackLWEBatch / UnpackLWEBatch (backend/packed.cpp:144-279):
 * 64-byte header ("LUXF", type LWE_BATCH = 2), u64 coefficients, sequential or INTERLEAVED (flag 1).
 * pack: out = NULL reports *size.  unpack: a/b = NULL report *n and *count. */
int fhe_hip_pack_lwe_batch(uint32_t n, size_t count, const uint64_t* a, const uint64_t* b, uint32_t flags,
                           uint8_t* out, size_t capacity, size_t* size);
int fhe_hip_unpack_lwe_batch(const uint8_t* data, size_t size, uint32_t* n, size_t* count, uint64_t* a, uint64_t* b);
/* ---- the reference's serialized objects: Serial::Serialize(obj, s, SerType::BINARY) streams
 * (utils/serial.h:95-125, cereal PortableBinary; binfhecontext-ser.h registrations) ----
 * RingGSWACCKey "refresh key" (cc.GetRefreshKey()) + LWESwitchingKey (cc.GetSwitchKey()): loaded
 * straight into the context (BTKeyLoad of deserialized keys, boolean-serial-binary.cpp flow). */
int fhe_hip_load_keys_cereal(fhe_hip_ctx* ctx, const uint8_t* refresh, size_t refresh_size, const uint8_t* sw,
                             size_t sw_size);
/* the same streams to / from the raw layouts (out = NULL reports the sizes) */
int fhe_hip_cereal_read_keys(int paramset, int method, const uint8_t* refresh, size_t refresh_size, const uint8_t* sw,
                             size_t sw_size, uint64_t* bsk, uint64_t* kskA, uint64_t* kskB);
int fhe_hip_cereal_write_keys(int paramset, int method, const uint64_t* bsk, size_t bsk_words, const uint64_t* kskA,
                              const uint64_t* kskB, uint8_t* refresh_out, size_t refresh_cap, size_t* refresh_size,
                              uint8_t* sw_out, size_t sw_cap, size_t* sw_size);
/* LWECiphertext (is_key = 0: a[n], b, modulus) or LWEPrivateKey (is_key = 1: s[n], modulus);
 * read with a = NULL reports *n */
int fhe_hip_cereal_read_lwe(const uint8_t* data, size_t size, int is_key, uint64_t* a, uint32_t cap_n, uint32_t* n,
                            uint64_t* b, uint64_t* mod);
int fhe_hip_cereal_write_lwe(const uint64_t* a, uint32_t n, uint64_t b, uint64_t mod, int is_key, uint8_t* out,
                             size_t cap, size_t* size);
/* The key-independent cryptoContext archive Serial::Serialize(BinFHEContext, BINARY) (boolean-serial-binary.cpp:
 * 65-71 writes it, :108 reads it back): BinFHEContext -> BinFHECryptoParams -> LWECryptoParams,
 * RingGSWCryptoParams (binfhecontext-ser.h:43,49,52-53).  read: the GenerateBinFHEContext(set, method) row
 * whose parameters the archive holds (the archive names none; FHE_HIP_ERR_INVALID_PARAM if no supported row
 * matches), with its parameters (out may be NULL).  write: the reference's bytes for a row (out = NULL
 * reports *size).  create_from_cereal: fhe_hip_create on the row a cryptoContext archive describes. */
int fhe_hip_cereal_read_context(const uint8_t* data, size_t size, int* paramset, int* method, fhe_hip_params* out);
int fhe_hip_cereal_write_context(int paramset, int method, uint8_t* out, size_t cap, size_t* size);
int fhe_hip_create_from_cereal(const uint8_t* data, size_t size, int device, fhe_hip_ctx** out);
/* EvalBinGate on two packed batches, result packed with out_flags (out = NULL reports *size) */
int fhe_hip_eval_bingate_packed(fhe_hip_ctx* ctx, int gate, const uint8_t* in1, size_t size1, const uint8_t* in2,
                                size_t size2, uint32_t out_flags, uint8_t* out, size_t capacity, size_t* size);
/* Packed keys: PackedBootstrappingKey (type 5) / PackedSwitchingKey (type 6) headers of
 * backend/packed.h (the reference's packers are TODO stubs, packed.cpp:284-328) followed by the
 * raw u64 layouts above; header.flags of the BSK = BINFHE_METHOD.  NULL outputs report sizes. */
int fhe_hip_pack_keys(int paramset, int method, const uint64_t* bsk, size_t bsk_words, const uint64_t* A,
                      const uint64_t* B, uint8_t* bsk_out, size_t bsk_cap, size_t* bsk_size, uint8_t* ksk_out,
                      size_t ksk_cap, size_t* ksk_size);
int fhe_hip_load_keys_packed(fhe_hip_ctx* ctx, const uint8_t* bsk, size_t bsk_size, const uint8_t* ksk,
                             size_t ksk_size);

/* EvalBinGate over count independent pairs (binfhe-base-scheme.cpp:76-126).
 * Inputs mod q, dimension n; outputs likewise.  ct1 and ct2 must not alias
 * (the reference's ct1 == ct2 check, :85-86, becomes a documented precondition). */
int fhe_hip_eval_bingate_batch(fhe_hip_ctx* ctx, int gate, size_t count, const uint64_t* a1, const uint64_t* b1,
                               const uint64_t* a2, const uint64_t* b2, uint64_t* a_out, uint64_t* b_out);
/* same on device buffers, asynchronous on stream (NULL = context stream) */
int fhe_hip_eval_bingate_batch_device(fhe_hip_ctx* ctx, int gate, size_t count, const uint64_t* d_a1,
                                      const uint64_t* d_b1, const uint64_t* d_a2, const uint64_t* d_b2,
                                      uint64_t* d_a_out, uint64_t* d_b_out, void* stream);
/* The two stages of fhe_hip_eval_bingate_batch_device, separately launchable:
 * blind_rotate leaves the mod-switched ctExt (N+1 values mod qKS per gate) in
 * the context's workspace; keyswitch consumes it (count must not exceed the
 * count of the last blind rotation: FHE_HIP_ERR_INVALID_PARAM otherwise). */
int fhe_hip_blind_rotate_batch_device(fhe_hip_ctx* ctx, int gate, size_t count, const uint64_t* d_a1,
                                      const uint64_t* d_b1, const uint64_t* d_a2, const uint64_t* d_b2, void* stream);
int fhe_hip_keyswitch_workspace_device(fhe_hip_ctx* ctx, size_t count, uint64_t* d_a_out, uint64_t* d_b_out,
                                       void* stream);
/* EvalBinGate(..., extended = true): ctExt before SwitchCTtoqn, dimension N, mod Q */
int fhe_hip_eval_bingate_extended(fhe_hip_ctx* ctx, int gate, size_t count, const uint64_t* a1, const uint64_t* b1,
                                  const uint64_t* a2, const uint64_t* b2, uint64_t* ext_a, uint64_t* ext_b);
/* EvalBinGate(gate, ctvector, extended) for gate in {MAJORITY, AND3, OR3, AND4, OR4}
 * (binfhe-base-scheme.cpp:129-171): k (2..4) inputs a_in[j] [count][n], b_in[j] [count]
 * mod q, summed; ptmod = the inputs' plaintext modulus (GetptModulus of ctvector[0]:
 * 6 for AND3/OR3, 8 for AND4/OR4, 4 for MAJORITY in the reference's tests).
 * extended = 0: outputs [count][n] mod q; extended = 1: ctExt [count][N] mod Q. */
int fhe_hip_eval_gate_multi_batch(fhe_hip_ctx* ctx, int gate, uint32_t k, uint32_t ptmod, size_t count,
                                  const uint64_t* const* a_in, const uint64_t* const* b_in, uint64_t* a_out,
                                  uint64_t* b_out, int extended);
int fhe_hip_eval_gate_multi_batch_device(fhe_hip_ctx* ctx, int gate, uint32_t k, uint32_t ptmod, size_t count,
                                         const uint64_t* const* d_a_in, const uint64_t* const* d_b_in,
                                         uint64_t* d_a_out, uint64_t* d_b_out, void* stream);
/* BinFHEContext::Bootstrap (binfhecontext.cpp; BinFHEScheme::Bootstrap, binfhe-base-scheme.cpp:190-218):
 * BootstrapGateCore(AND, ct + q/4), extraction (b = Q/8 + 1 + acc1[0]) and SwitchCTtoqn -- the refresh of
 * lux_fhe_bootstrap (c_api.cpp:263-276).  Ciphertexts a[count][n], b[count] mod q, plaintext modulus 4. */
int fhe_hip_bootstrap_batch(fhe_hip_ctx* ctx, size_t count, const uint64_t* a, const uint64_t* b, uint64_t* a_out,
                            uint64_t* b_out);
int fhe_hip_bootstrap_batch_device(fhe_hip_ctx* ctx, size_t count, const uint64_t* d_a, const uint64_t* d_b,
                                   uint64_t* d_a_out, uint64_t* d_b_out, void* stream);
/* EvalBinGate(CMUX, {ct0, ct1, ct2}) = NAND(NAND(ct0, NOT ct2), NAND(ct1, ct2)), i.e. ct2 ? ct1 : ct0
 * (binfhe-base-scheme.cpp:172-182; EvalCMUXBatch, batch.cpp:212-249, passes {sel, true, false}). */
int fhe_hip_eval_cmux_batch(fhe_hip_ctx* ctx, size_t count, const uint64_t* a0, const uint64_t* b0,
                            const uint64_t* a1, const uint64_t* b1, const uint64_t* a2, const uint64_t* b2,
                            uint64_t* a_out, uint64_t* b_out);
int fhe_hip_eval_cmux_batch_device(fhe_hip_ctx* ctx, size_t count, const uint64_t* d_a0, const uint64_t* d_b0,
                                   const uint64_t* d_a1, const uint64_t* d_b1, const uint64_t* d_a2,
                                   const uint64_t* d_b2, uint64_t* d_a_out, uint64_t* d_b_out, void* stream);
/* ---- ciphertexts mod Q (extended outputs, LARGE_DIM encryptions) as inputs ----
 * BinFHEScheme::EvalBinGate / EvalBinGate(ctvector) / Bootstrap switch every input whose modulus is Q
 * to (n, q) first (binfhe-base-scheme.cpp:92-93, 150-152, 200: SwitchCTtoqn), and inputs of either
 * modulus may be mixed within one call.
 * SwitchCTtoqn (lwe-pke.cpp:170-178; BinFHEContext::SwitchCTtoqn, binfhecontext.cpp:254-264):
 *   a[count][N], b[count] mod Q -> a_out[count][n], b_out[count] mod q. */
int fhe_hip_switch_to_qn_batch(fhe_hip_ctx* ctx, size_t count, const uint64_t* a, const uint64_t* b, uint64_t* a_out,
                               uint64_t* b_out);
int fhe_hip_switch_to_qn_batch_device(fhe_hip_ctx* ctx, size_t count, const uint64_t* d_a, const uint64_t* d_b,
                                      uint64_t* d_a_out, uint64_t* d_b_out, void* stream);
/* op: OR..XNOR / XOR_FAST / XNOR_FAST (k = 2; EvalBinGate(gate, ct1, ct2, extended), :76-126),
 * MAJORITY / AND3 / OR3 / AND4 / OR4 (k = 2..4, inputs' plaintext modulus ptmod; :129-175), CMUX (k = 3,
 * {ct0, ct1, ct2} -> ct2 ? ct1 : ct0, extended ignored as the reference ignores it, :176-182), or
 * FHE_HIP_OP_BOOTSTRAP (k = 1, Bootstrap(ct, extended), :190-220, the input's plaintext modulus ptmod).
 * Column j: count ciphertexts a_in[j], b_in[j]; large == NULL or large[j] == NULL: rows of n words, all mod q;
 * otherwise rows of N words, large[j][g] = 1 marking a ciphertext mod Q (dimension N), 0 one mod q (its first
 * n words used).  Outputs [count][n] mod q, or ctExt [count][N] mod Q when extended.
 * Bootstrap of an input mod Q keeps the reference's constant ct->GetModulus() >> 2 (:201), added at q by
 * ModAddFast, so its test vector is the window's constant uv.  That shortcut needs
 * Q / 4 >= 2.5 q, true for every parameter row (the smallest ratio is far above it); a set below it is refused
 * with FHE_HIP_ERR_INVALID_PARAM rather than computed differently from the reference. */
#define FHE_HIP_OP_BOOTSTRAP (-1)
int fhe_hip_eval_mixed_batch(fhe_hip_ctx* ctx, int op, uint32_t k, uint32_t ptmod, size_t count,
                             const uint64_t* const* a_in, const uint64_t* const* b_in, const uint8_t* const* large,
                             uint64_t* a_out, uint64_t* b_out, int extended);
/* device buffers (large[j] device arrays too), asynchronous on stream */
int fhe_hip_eval_mixed_batch_device(fhe_hip_ctx* ctx, int op, uint32_t k, uint32_t ptmod, size_t count,
                                    const uint64_t* const* d_a_in, const uint64_t* const* d_b_in,
                                    const uint8_t* const* d_large, uint64_t* d_a_out, uint64_t* d_b_out, int extended,
                                    void* stream);

/* ---- functional bootstrapping (binfhe-base-scheme.cpp:241-521, 589-648) ----
 * Batches of `count` LWE ciphertexts a[count][n], b[count] under the context's keys; beta = 128
 * (BinFHEContext::GetBeta).  Moduli are powers of two.
 * EvalFunc (binfhecontext.cpp:340-344): inputs/outputs mod q_in; lut[lut_len = q_in] as from
 *   GenerateLUTviaFunction; negacyclic / periodic / arbitrary LUTs as checkInputFunction
 *   classifies them (arbitrary needs q_in <= N). */
int fhe_hip_eval_func_batch(fhe_hip_ctx* ctx, size_t count, const uint64_t* a, const uint64_t* b, uint64_t q_in,
                            const uint64_t* lut, size_t lut_len, uint64_t* a_out, uint64_t* b_out);
int fhe_hip_eval_func_batch_device(fhe_hip_ctx* ctx, size_t count, const uint64_t* d_a, const uint64_t* d_b,
                                   uint64_t q_in, const uint64_t* lut, size_t lut_len, uint64_t* d_a_out,
                                   uint64_t* d_b_out, void* stream);
/* EvalFuncMultiOutputBatch (batch.cpp:141-174): EvalFunc(ct_i, luts[j]) for every input i and each of num_luts
 * LUTs luts[num_luts][lut_len = q_in]; output j of input i at row i * num_luts + j of a_out [count * num_luts][n],
 * b_out [count * num_luts].  The LUT-independent first bootstrap of EvalFunc's periodic / arbitrary forms runs
 * once per input and class; the LUT-dependent last bootstraps of a class run as one launch. */
int fhe_hip_eval_func_multi_batch(fhe_hip_ctx* ctx, size_t count, const uint64_t* a, const uint64_t* b, uint64_t q_in,
                                  const uint64_t* luts, size_t lut_len, uint32_t num_luts, uint64_t* a_out,
                                  uint64_t* b_out);
int fhe_hip_eval_func_multi_batch_device(fhe_hip_ctx* ctx, size_t count, const uint64_t* d_a, const uint64_t* d_b,
                                         uint64_t q_in, const uint64_t* luts, size_t lut_len, uint32_t num_luts,
                                         uint64_t* d_a_out, uint64_t* d_b_out, void* stream);
/* EvalFloor (binfhecontext.cpp:346-357): inputs/outputs mod `mod` (<= 2^31) */
int fhe_hip_eval_floor_batch(fhe_hip_ctx* ctx, size_t count, const uint64_t* a, const uint64_t* b, uint64_t mod,
                             uint32_t roundbits, uint64_t* a_out, uint64_t* b_out);
/* EvalSign (binfhecontext.cpp:359-364): inputs mod `mod` (q < mod <= 2^31), outputs mod q */
int fhe_hip_eval_sign_batch(fhe_hip_ctx* ctx, size_t count, const uint64_t* a, const uint64_t* b, uint64_t mod,
                            int scheme_switch, uint64_t* a_out, uint64_t* b_out);
/* EvalDecomp (binfhecontext.cpp:366-370): *parts ciphertexts per input; a_out [parts][count][n],
 * b_out [parts][count]; parts - 1 of them mod q, the last one mod its own reduced modulus */
int fhe_hip_eval_decomp_parts(fhe_hip_ctx* ctx, uint64_t mod, uint32_t* parts);
int fhe_hip_eval_decomp_batch(fhe_hip_ctx* ctx, size_t count, const uint64_t* a, const uint64_t* b, uint64_t mod,
                              uint64_t* a_out, uint64_t* b_out);
/* BootstrapFunc (binfhe-base-scheme.cpp:617-642): a mod ctmod (<= 2N), f[ctmod] with f(x) <= fmod,
 * outputs mod fmod (<= 2^40) */
int fhe_hip_bootstrap_func_batch(fhe_hip_ctx* ctx, size_t count, const uint64_t* a, const uint64_t* b,
                                 uint32_t ctmod, const uint64_t* f, uint64_t fmod, uint64_t* a_out, uint64_t* b_out);

/* ---- the reference GPU seam lux::fhe::backend::Backend (src/binfhe/include/backend/backend.h) ----
 * Backend::BlindRotate / BlindRotateBatch (backend.h:131-136, 177-182) = the accumulator's EvalAcc
 * (rgsw-acc-cggi.cpp:59-68, rgsw-acc-lmkcdey.cpp:70-158, rgsw-acc-dm.cpp:62-77) on `count` pairs:
 * a[count][n] mod ctmod (the LWE ciphertext's modulus: a power of two <= 2N; 2N for LMKCDEY, q for
 * AP), acc[count][2][N] in/out (RLWECiphertext elements 0 and 1, EVALUATION, bit-reversed as the
 * reference stores them, canonical mod Q).  Every parameter set and method of the context. */
int fhe_hip_blind_rotate_acc_batch(fhe_hip_ctx* ctx, size_t count, const uint64_t* a, uint64_t ctmod, uint64_t* acc);
int fhe_hip_blind_rotate_acc_batch_device(fhe_hip_ctx* ctx, size_t count, const uint64_t* d_a, uint64_t ctmod,
                                          uint64_t* d_acc, void* stream);
/* BlindRotateBatch with null accumulators -- what BootstrapBatch (batch/batch.cpp:53-104) passes
 * ("initialize accumulators with LUT (identity for bootstrap)", :77-86): the accumulator of
 * BinFHEScheme::Bootstrap (binfhe-base-scheme.cpp:190-205), i.e. BootstrapGateCore(AND, ct + q/4)
 * (:525-583): the AND window's test vector at b + q/4, NTT'd, then EvalAcc over a.  Ciphertexts
 * a[count][n], b[count] mod q; acc[count][2][N] out (EVALUATION, canonical mod Q). */
int fhe_hip_blind_rotate_init_batch(fhe_hip_ctx* ctx, size_t count, const uint64_t* a, const uint64_t* b,
                                    uint64_t* acc);
int fhe_hip_blind_rotate_init_batch_device(fhe_hip_ctx* ctx, size_t count, const uint64_t* d_a, const uint64_t* d_b,
                                           uint64_t* d_acc, void* stream);
/* Backend::ExternalProduct / ExternalProductBatch (backend.h:141-146, 187-192): RGSW x RLWE -> RLWE,
 * result[g] = sum_d D_d(rlwe[g]) * rgsw[g][d] with D = SignedDigitDecompose (rgsw-acc.cpp:54-91) --
 * AddToAccLMKCDEY / AddToAccDM (rgsw-acc-lmkcdey.cpp:228-254, rgsw-acc-dm.cpp:119-145) under the
 * context's baseG.  rgsw[count][digitsG2][2][N] (RingGSWEvalKeyImpl rows, EVALUATION), rlwe and
 * result [count][2][N] (EVALUATION), canonical mod Q; result may equal rlwe. */
int fhe_hip_external_product_batch(fhe_hip_ctx* ctx, size_t count, const uint64_t* rgsw, const uint64_t* rlwe,
                                   uint64_t* result);
int fhe_hip_external_product_batch_device(fhe_hip_ctx* ctx, size_t count, const uint64_t* d_rgsw,
                                          const uint64_t* d_rlwe, uint64_t* d_result, void* stream);
/* Backend::MaxBatchSize (backend.h:86): gates one call can take given the device's free memory */
int fhe_hip_max_batch_size(fhe_hip_ctx* ctx, size_t* max_count);
/* Backend::UnpackBootstrappingKey (backend.h:229-233): packed keys (fhe_hip_pack_keys) back to the
 * raw layouts; either key may be skipped (NULL); *_cap = the output buffers' sizes in u64 words
 * (FHE_HIP_ERR_INVALID_PARAM when too small) */
int fhe_hip_unpack_keys(int paramset, int method, const uint8_t* bsk_packed, size_t bsk_size, uint64_t* bsk,
                        size_t bsk_cap, const uint8_t* ksk_packed, size_t ksk_size, uint64_t* kskA, size_t kskA_cap,
                        uint64_t* kskB, size_t kskB_cap);

/* ---- boolean circuits: the reference's BatchDAG (src/binfhe/include/batch/binfhe-batch.h:229-279), whose
 * Execute runs one gate at a time (src/binfhe/lib/batch/batch.cpp:429-482) ----
 * A circuit is a DAG built on the host (no context, no device).  Nodes get consecutive ids from 0 in the order
 * they are added, returned in *id; operands must be existing ids.
 *   input      a circuit input (a ciphertext mod q, dimension n)
 *   not        EvalNOT (binfhe-base-scheme.cpp:223-236): costs no bootstrap, folded into its users
 *   gate       OR, AND, NOR, NAND, XOR, XNOR, XOR_FAST, XNOR_FAST on two nodes
 *   gate_multi MAJORITY, AND3, OR3, AND4, OR4 on 2 to 4 nodes at a plaintext modulus p (EvalBinGate(gate, ctvector),
 *              :127-170): one bootstrap
 *   cmux       sel ? c1 : c0 = NAND(NAND(c0, NOT sel), NAND(c1, sel)) (:172-182): three bootstraps, two levels
 *   bootstrap  BinFHEScheme::Bootstrap (:190-218)
 *   func       EvalFunc(x, lut) (:241-337): one bootstrap for a negacyclic LUT, two for a periodic or an arbitrary
 *              one (two levels); FUNC nodes of one class on one operand share the first of the two
 *   linear     sum of 1 to 4 nodes with signs, plus a constant on b, mod q (EvalAddEq / EvalSubEq /
 *              EvalAddConstEq, lwe-pke.cpp:230-246): no bootstrap, a row of its own at its operands' highest level
 * Any node can be marked as an output, any number of times; outputs come back in marking order.
 * finalize levelises the DAG (inputs level 0; a bootstrapped node one more than its operands' highest level; a
 * NOT the level of its source) and gives every level's nodes one contiguous block of rows in the evaluation's
 * ciphertext pool (inputs first).  Evaluation runs level by level: one prep + blind rotation + key switch over
 * ALL gates of a level, whatever their types (the multi-input gates at p = 4 among them), times `count` independent
 * instances, one more such launch for the level's FUNC bootstraps at modulus q, one for those at 2q and one per
 * other plaintext modulus of its multi-input gates, then one element-wise launch for its linear nodes
 * (DESIGN.md §4 "Circuits").
 * Not supported: inputs mod Q (every input is a ciphertext mod q of dimension n).
 * Errors: FHE_HIP_ERR_INVALID_PARAM for an unknown id, an unsupported gate code, gate(g, x, x) on the same
 * (node, negation) -- the reference's ct1 == ct2 check (:85-86); gate(AND, x, not x) is accepted -- and any add /
 * mark_output / finalize on a finalized circuit; FHE_HIP_ERR_NOT_INIT for a plan query or an evaluation before
 * finalize. */
typedef struct fhe_hip_circuit fhe_hip_circuit;
int fhe_hip_circuit_create(fhe_hip_circuit** out);
void fhe_hip_circuit_destroy(fhe_hip_circuit* c);
int fhe_hip_circuit_add_input(fhe_hip_circuit* c, uint32_t* id);
int fhe_hip_circuit_add_not(fhe_hip_circuit* c, uint32_t x, uint32_t* id);
int fhe_hip_circuit_add_gate(fhe_hip_circuit* c, int gate, uint32_t x, uint32_t y, uint32_t* id);
/* gate = MAJORITY, AND3, OR3, AND4 or OR4 over the k nodes xs, 2 <= k <= 4 for every code (the rule of
 * fhe_hip_eval_gate_multi_batch; the reference sums the vector it is given), at plaintext modulus ptmod >= 2.  An
 * operand may be any node; one that resolves to a NOT folds in as a sign flip and q/4, which equals the per-gate
 * entry fed the EvalNOT of that operand.  Encodings are not type-checked (the reference takes p from ctvector[0]):
 * the caller owns the plaintext modulus of what it wires together, and only p = 4 nodes compose with 2-input
 * gates and NOT.  Nodes at ptmod = 4 share the level's gate launch; every other modulus in a level is one more
 * launch, and any number of moduli may be mixed.  FHE_HIP_ERR_INVALID_PARAM for any other gate code, k out of
 * range, an unknown id, ptmod < 2, or two operands on one (node, negation) -- the reference's pairwise check
 * (:136-143); (x, not x, y) is accepted.  2 ptmod > q is only known at evaluation, which refuses with
 * FHE_HIP_ERR_INVALID_PARAM before anything is touched.  fhe_hip_circuit_add_gate keeps refusing these codes. */
int fhe_hip_circuit_add_gate_multi(fhe_hip_circuit* c, int gate, const uint32_t* xs, uint32_t k, uint32_t ptmod,
                                   uint32_t* id);
int fhe_hip_circuit_add_cmux(fhe_hip_circuit* c, uint32_t c0, uint32_t c1, uint32_t sel, uint32_t* id);
int fhe_hip_circuit_add_bootstrap(fhe_hip_circuit* c, uint32_t x, uint32_t* id);
/* lut[len], len a power of two >= 4, every value < len.  FHE_HIP_ERR_INVALID_PARAM otherwise, and when x resolves to
 * a NOT (EvalNOT negates mod q, which does not survive an arbitrary LUT's lift to 2q: bootstrap it, or fold the
 * NOT into the LUT).  The LUT's class (checkInputFunction, binfhe-base-scheme.h:245-260) is fixed here.  len must
 * equal the evaluating context's q, and an arbitrary LUT needs q <= N and a method other than AP: both are only
 * known at evaluation, which refuses with FHE_HIP_ERR_INVALID_PARAM. */
int fhe_hip_circuit_add_func(fhe_hip_circuit* c, uint32_t x, const uint64_t* lut, size_t len, uint32_t* id);
/* sum_j (signs[j] < 0 ? -1 : +1) xs[j] + (0, constant mod q), 1 <= k <= 4; signs NULL: all +.  An operand that
 * resolves to a NOT folds in as a sign flip and +-q/4.  FHE_HIP_ERR_INVALID_PARAM for k out of range, an unknown
 * id, or an operand that is itself a linear node (flatten the sum). */
int fhe_hip_circuit_add_linear(fhe_hip_circuit* c, const uint32_t* xs, const int* signs, uint32_t k, uint64_t constant,
                               uint32_t* id);
int fhe_hip_circuit_mark_output(fhe_hip_circuit* c, uint32_t id);
int fhe_hip_circuit_finalize(fhe_hip_circuit* c);
/* slots (gates x instances) per launch: 0 = fhe_hip_max_batch_size; a smaller value cuts wider levels into
 * contiguous chunks of slots (results are the same).  May be changed between evaluations. */
int fhe_hip_circuit_set_max_slots(fhe_hip_circuit* c, size_t max_slots);
/* any pointer may be NULL; n_levels (bootstrapped levels, the inputs' level 0 not counted) and n_bootstraps need a
 * finalized circuit */
int fhe_hip_circuit_counts(const fhe_hip_circuit* c, size_t* n_inputs, size_t* n_outputs, size_t* n_levels,
                           size_t* n_bootstraps);
/* level 0 .. n_levels (0: the inputs): its number of nodes and the pool row of its first node */
int fhe_hip_circuit_level(const fhe_hip_circuit* c, size_t level, size_t* width, size_t* first_row);
/* A level's rows in row order: widths[0..2] its bootstraps by launch class (0 gates, BOOTSTRAP and the multi-input
 * gates at p = 4, 1 tables at q, 2 tables at 2q with the first stages first; each class one contiguous block),
 * widths[3] its linear rows.  Between class 2 and the linear rows lie the gate classes of the other plaintext
 * moduli (below); fhe_hip_circuit_level's width counts them.  Level 0 holds the inputs (not counted here) and its
 * linear rows. */
int fhe_hip_circuit_level_classes(const fhe_hip_circuit* c, size_t level, size_t widths[4]);
/* The level's gate classes of plaintext moduli other than 4, in row order (ascending modulus): *n_classes pairs
 * (ptmods[i], widths[i]).  Either array may be NULL; otherwise cap (entries) must hold them. */
int fhe_hip_circuit_level_gate_classes(const fhe_hip_circuit* c, size_t level, uint32_t* ptmods, size_t* widths,
                                       size_t cap, size_t* n_classes);
/* *cls = 0 negacyclic, 1 periodic, 2 arbitrary for a func node, -1 for any other; known as soon as it is added */
int fhe_hip_circuit_func_class(const fhe_hip_circuit* c, uint32_t id, int* cls);
/* The distinct test-vector tables launch class cls (1 or 2) holds for a parameter set (host only): *n_tables
 * tables of *ctmod (q or 2q) words, (Q / ctmod) f(x) as BootstrapFuncCore scales them (:596-608).  out may be NULL
 * to size it; otherwise cap (words) must hold them.  FHE_HIP_ERR_INVALID_PARAM as at evaluation (above). */
int fhe_hip_circuit_tables(const fhe_hip_circuit* c, int paramset, int method, int cls, uint64_t* out, size_t cap,
                           size_t* n_tables, size_t* ctmod);
/* the pool row node id resolves to, and whether it is that row's EvalNOT (a NOT chain collapses onto its source) */
int fhe_hip_circuit_node_row(const fhe_hip_circuit* c, uint32_t id, uint32_t* row, uint32_t* negated);
/* `count` independent instances of the circuit.  a_in [n_in][count][n], b_in [n_in][count] mod q (input j =
 * the j-th add_input); a_out [n_out][count][n], b_out [n_out][count].  n_in / n_out must be the circuit's counts.
 * The circuit is checked before the context (NULL circuit, not finalized, wrong counts), so those refusals need
 * no device.  FHE_HIP_ERR_ALLOC when the pool ((n_in + bootstraps + linear nodes) * count ciphertexts; rows are not reused)
 * would not fit the device's free memory (fhe_hip_device_memory). */
int fhe_hip_eval_circuit_batch(fhe_hip_ctx* ctx, const fhe_hip_circuit* c, size_t count, uint32_t n_in,
                               const uint64_t* a_in, const uint64_t* b_in, uint32_t n_out, uint64_t* a_out,
                               uint64_t* b_out);
/* device buffers, asynchronous on stream: every level is enqueued with no host synchronisation in between */
int fhe_hip_eval_circuit_batch_device(fhe_hip_ctx* ctx, const fhe_hip_circuit* c, size_t count, uint32_t n_in,
                                      const uint64_t* d_a_in, const uint64_t* d_b_in, uint32_t n_out,
                                      uint64_t* d_a_out, uint64_t* d_b_out, void* stream);
/* How a level's gates share one launch (host only): gate's q1 = GetGateConst (rgsw-cryptoparameters.cpp:78-92),
 * whether its input sum is doubled (XOR / XNOR), and bshift = q1(ref_gate) - q1(gate) mod q.  BootstrapGateCore's
 * test vector (:535-567) of `gate` at b equals that of ref_gate at b + bshift, because the six 2-input gates
 * differ only in where the half-circle window [q1, q1 + q/2) starts. */
int fhe_hip_gate_fold(int paramset, int method, int gate, int ref_gate, uint32_t* dbl, uint64_t* bshift, uint64_t* q1);
/* BootstrapGateCore's window (:535-556) of any gate but CMUX at plaintext modulus ptmod (host only): its start q1,
 * the value Q/(2 ptmod) + 1 of the test vector, the b the extraction adds (that value for the multi-input gates,
 * :162; (Q >> 3) + 1 for a 2-input gate whatever ptmod, :118) and bshift_to_and = q1(AND) - q1(gate) mod q.  Every
 * gate's window is the half circle [q1, q1 + q/2), so the fold above holds for the multi-input gates too; launches
 * differ only in *value.  MAJORITY at ptmod = 4 equals AND in all four.  FHE_HIP_ERR_INVALID_PARAM for CMUX, an
 * unknown code, ptmod < 2 or 2 ptmod > q. */
int fhe_hip_gate_window(int paramset, int method, int gate, uint32_t ptmod, uint64_t* q1, uint64_t* value,
                        uint64_t* b_const, uint64_t* bshift_to_and);

/* LWEEncryptionScheme::KeySwitch (lwe-pke.cpp:348-372): (N, qKS) -> (n, qKS) */
int fhe_hip_keyswitch_batch(fhe_hip_ctx* ctx, size_t count, const uint64_t* a, const uint64_t* b, uint64_t* a_out,
                            uint64_t* b_out);
/* LWEEncryptionScheme::ModSwitch (lwe-pke.cpp:254-261): RoundqQ in IEEE double exactly as the
 * reference evaluates it (lwe-pke.cpp:41-46), for any nonzero moduli */
int fhe_hip_modswitch_batch(fhe_hip_ctx* ctx, uint64_t q_from, uint64_t q_to, uint32_t len, size_t count,
                            const uint64_t* a, const uint64_t* b, uint64_t* a_out, uint64_t* b_out);

/* Single-process multi-device: one host thread + stream per device,
 * contiguous shards, keys replicated on every device, no collectives.
 * devices may repeat (several contexts on one GPU). */
typedef struct fhe_hip_multi fhe_hip_multi;
int fhe_hip_multi_create(int paramset, int method, const int* devices, int ndev, fhe_hip_multi** out);
void fhe_hip_multi_destroy(fhe_hip_multi* m);
int fhe_hip_multi_load_keys(fhe_hip_multi* m, const uint64_t* bsk, size_t n_words, const uint64_t* A, size_t nA,
                            const uint64_t* B, size_t nB);
int fhe_hip_multi_eval_bingate_batch(fhe_hip_multi* m, int gate, size_t count, const uint64_t* a1, const uint64_t* b1,
                                     const uint64_t* a2, const uint64_t* b2, uint64_t* a_out, uint64_t* b_out);

/* ------------------------------------------------------------------------ */
/* Deterministic host key material (KeyGen / BTKeyGen / Encrypt / Decrypt,   */
/*   binfhecontext.cpp:185-307) -- seeded, same structure as the reference. */
/* ------------------------------------------------------------------------ */
/* KeyGen (binfhecontext.cpp:185-190): sk[n] (mod qKS) only */
int fhe_hip_keygen_secret(int paramset, int method, uint64_t seed, uint64_t* sk);
/* sk[n] (mod qKS), bsk[bsk_words], kskA[ksk_rows*n], kskB[ksk_rows] */
int fhe_hip_keygen(int paramset, int method, uint64_t seed, uint64_t* sk, uint64_t* bsk, uint64_t* kskA,
                   uint64_t* kskB);
/* a[count][n], b[count] mod q, plaintext modulus 4 */
int fhe_hip_encrypt(int paramset, int method, const uint64_t* sk, const int* bits, size_t count, uint64_t seed,
                    uint64_t* a, uint64_t* b);
int fhe_hip_decrypt(int paramset, int method, const uint64_t* sk, const uint64_t* a, const uint64_t* b, size_t count,
                    uint32_t len, uint64_t mod, int64_t* out);
/* the same with an explicit plaintext modulus (Encrypt/Decrypt(..., p), lwe-pke.cpp:103-128, 181-226) */
int fhe_hip_encrypt_ptmod(int paramset, int method, const uint64_t* sk, const int* bits, size_t count, uint64_t seed,
                          uint32_t ptmod, uint64_t* a, uint64_t* b);
/* ... and an explicit ciphertext modulus mod (Encrypt(sk, m, SMALL_DIM, p, mod), binfhecontext.cpp:220-234) */
int fhe_hip_encrypt_mod(int paramset, int method, const uint64_t* sk, const int* bits, size_t count, uint64_t seed,
                        uint32_t ptmod, uint64_t mod, uint64_t* a, uint64_t* b);
int fhe_hip_decrypt_ptmod(int paramset, int method, const uint64_t* sk, const uint64_t* a, const uint64_t* b,
                          size_t count, uint32_t len, uint64_t mod, uint32_t ptmod, int64_t* out);
/* The RLWE secret skN[N] of fhe_hip_keygen(..., seed, ...) (KeyGenN's key, binfhecontext.cpp:203-208), stored
 * mod qKS as the key switch holds it (lwe-pke.cpp:285-286): the LWE secret of dimension-N ciphertexts mod Q.
 * fhe_hip_decrypt_ptmod with len = N, mod = Q decrypts them under it. */
int fhe_hip_keygen_ring_secret(int paramset, int method, uint64_t seed, uint64_t* skN);
/* Encrypt(pk, m, LARGE_DIM, p) (binfhecontext.cpp:236-252, EncryptN): a[count][N], b[count] mod Q under skN
 * (a symmetric encryption under the key the public key belongs to; uniform a, the reference's Gaussian; the
 * public-key form itself is fhe_hip_encrypt_pk below) */
int fhe_hip_encrypt_large(int paramset, int method, const uint64_t* skN, const int* bits, size_t count, uint64_t seed,
                          uint32_t ptmod, uint64_t* a, uint64_t* b);

/* ------------------------------------------------------------------------ */
/* Public-key encryption (KeyGenPair / PubKeyGen lwe-pke.cpp:59-98, EncryptN */
/*   lwe-pke.cpp:133-167, Encrypt(pk, ..) binfhecontext.cpp:236-252)         */
/* ------------------------------------------------------------------------ */
/* PubKeyGen (lwe-pke.cpp:74-98) for the ring secret skN[N] (mod qKS, as fhe_hip_keygen_ring_secret returns it):
 * A[N][N] row-major uniform mod Q, v[j] = e_j + <A[j], s> mod Q.  With skN = fhe_hip_keygen_ring_secret(seed) the
 * key belongs to the keys fhe_hip_keygen / fhe_hip_btkeygen_device make from that seed (with timeOptimization: to
 * the key of the context's own baseG, as m_BTKey.Pkey does, binfhe-base-scheme.cpp:53-57). */
int fhe_hip_pubkeygen(int paramset, int method, const uint64_t* skN, uint64_t seed, uint64_t* A, uint64_t* v);
/* the errors e[N] of fhe_hip_pubkeygen(seed) as signed values (draw j of its error stream) */
int fhe_hip_pubkeygen_draws(int paramset, int method, uint64_t seed, int64_t* e);
/* EncryptN (lwe-pke.cpp:133-167) with ciphertext modulus Q: a[count][N], b[count];
 * a_i = e'_i + sum_j s'_j A[j][i] (:151-154), b = (m mod ptmod) floor(Q / ptmod) + e'' + sum_j v[j] s'_j (:158-162),
 * s' uniform ternary.  Ciphertext g depends on (seed, first + g) only: a batch cut into several calls, or sharded
 * over devices, gives the same ciphertexts.  FHE_HIP_ERR_INVALID_PARAM for ptmod < 2 or ptmod > Q. */
int fhe_hip_encrypt_pk(int paramset, int method, const uint64_t* A, const uint64_t* v, const int* bits, size_t count,
                       uint64_t first, uint64_t seed, uint32_t ptmod, uint64_t* a, uint64_t* b);
/* The draws of ciphertexts [first, first + count) of fhe_hip_encrypt_pk as signed values: sp[count][N] (s'),
 * ep[count][N] (e'), epp[count] (e'') */
int fhe_hip_encrypt_pk_draws(int paramset, int method, size_t count, uint64_t first, uint64_t seed, int64_t* sp,
                             int64_t* ep, int64_t* epp);
/* The public key made resident on the context's device (A[N][N], v[N], reduced mod Q) */
int fhe_hip_load_pubkey(fhe_hip_ctx* ctx, const uint64_t* A, const uint64_t* v);
/* PubKeyGen on the device: the key fhe_hip_pubkeygen(skN, seed) makes, bit for bit, generated in place in the
 * resident layout; A_out / v_out (either may be NULL) receive it.  N must be the set's ring dimension. */
int fhe_hip_pubkeygen_device(fhe_hip_ctx* ctx, const uint64_t* skN, size_t N, uint64_t seed, uint64_t* A_out,
                             uint64_t* v_out);
/* Encrypt(pk, m, output, p) (binfhecontext.cpp:236-252) of bits[count] under the resident public key, the
 * ciphertexts fhe_hip_encrypt_pk makes for (first, seed), bit for bit.  output 3 (LARGE_DIM): a_out[count][N],
 * b_out[count] mod Q, the row layout fhe_hip_eval_mixed_batch reads as "large"; 4 (SMALL_DIM): SwitchCTtoqn of
 * those (:246-249), a_out[count][n], b_out[count] mod q.  FHE_HIP_ERR_INVALID_PARAM for ptmod < 2, ptmod > Q or
 * another output; FHE_HIP_ERR_NOT_INIT without a resident public key (SMALL_DIM: or switching key); count = 0
 * is a no-op. */
#define FHE_HIP_LARGE_DIM 3
#define FHE_HIP_SMALL_DIM 4
int fhe_hip_encrypt_pk_batch(fhe_hip_ctx* ctx, const int* bits, size_t count, uint64_t first, uint64_t seed,
                             uint32_t ptmod, int output, uint64_t* a_out, uint64_t* b_out);
/* The same on device buffers (d_bits: int32), asynchronous on stream and ordered with the context's other calls */
int fhe_hip_encrypt_pk_batch_device(fhe_hip_ctx* ctx, const int* d_bits, size_t count, uint64_t first, uint64_t seed,
                                    uint32_t ptmod, int output, uint64_t* d_a_out, uint64_t* d_b_out, void* stream);
/* ciphertexts per workgroup of the EncryptN kernel (batch sizes around its multiples are the tile edges) */
uint32_t fhe_hip_encrypt_pk_tile(void);

/* ------------------------------------------------------------------------ */
/* Device memory (Backend::Allocate/Free/CopyToDevice/CopyToHost/Synchronize, */
/*   backend.h:94-114)                                                       */
/* ------------------------------------------------------------------------ */
int fhe_hip_alloc(int device, size_t bytes, void** d_ptr);
int fhe_hip_free(void* d_ptr);
int fhe_hip_copy_to_device(void* d_dst, const void* h_src, size_t bytes);
int fhe_hip_copy_to_host(void* h_dst, const void* d_src, size_t bytes);
int fhe_hip_synchronize(int device);
int fhe_hip_device_count(int* count);
/* Backend::DeviceMemory (backend.h:87): free / total bytes of the device (either may be NULL) */
int fhe_hip_device_memory(int device, size_t* free_bytes, size_t* total_bytes);
/* Table check of the fused accumulator kernels' signed forward transform (host only, no device): with
 * t1, t2, t3 = Table[1..3] of the negacyclic NTT mod the odd prime Q (plain residues), the constants
 * c+- = (t2 +- t1 t2) / 2 mod Q of its first 4-point group.  FHE_HIP_ERR_INVALID_PARAM unless t1^2 = -1 and
 * t3 = t1 t2 mod Q -- the check the context's table builder makes before any kernel can run. */
int fhe_hip_fwd_group_consts(uint64_t Q, uint64_t t1, uint64_t t2, uint64_t t3, uint64_t* c_plus, uint64_t* c_minus);
/* Product twiddles of two transform stages the fused accumulator kernel takes as one 4-point group (host only):
 * with t1 = Table[1], w1 = Table[k], w2 = Table[2k], w3 = Table[2k + 1] (plain residues), w12 = w1 w2 and
 * w13n = -(w1 w3) mod Q.  FHE_HIP_ERR_INVALID_PARAM unless t1^2 = -1, w2^2 = w1 and w3 = t1 w2 mod Q.
 * fhe_hip_stage_group_table: the 328 products of one direction from its bit-reversed table of n = 1024 entries,
 * 8 wave-uniform ones, then 10 x 32 lane-major ones, in the order the table builder uploads them; refused as soon
 * as one triple fails the check above. */
int fhe_hip_stage_group_consts(uint64_t Q, uint64_t t1, uint64_t w1, uint64_t w2, uint64_t w3, uint64_t* w12,
                               uint64_t* w13n);
int fhe_hip_stage_group_table(uint64_t Q, const uint64_t* table, size_t n, uint64_t* out, size_t out_cap);
/* message of the last error on this host thread */
const char* fhe_hip_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* FHE_HIP_H */
