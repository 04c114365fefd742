// keygen_desc.h -- the row-pair descriptors of device BTKeyGen (keygen_dev_wide.hip) and the plan query built on
// them (fhe_hip_keygen_plan_get).  Host only: no device is needed to build or count them.
//
// One descriptor per RGSW row pair, in the order keygen_one() (keygen.cpp) draws them, with its (stream, call)
// numbering: GINX [i][ks][row], AP [i][k][j >= 1][row] at slot (i baseR + j) digitsR + k, LMKCDEY [i][row] then the
// automorphism keys [k][row].  Row pair `row` of a key starts at draw row * 2N of the key's stream: N uniform draws
// (the mask A) and N Gaussian draws (the error e).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "params.h"

namespace fhe_amd {

struct KgRow {
    uint64_t s0;    // rng_state of the stream
    uint64_t mval;  // message mval * X^mm mod Q (0: none)
    uint64_t g;     // automorphism key: its gadget power
    uint32_t rp;    // row pair: words [rp * 2N, (rp + 1) * 2N) of the raw key
    uint32_t call;  // first draw of this row pair in the stream
    uint32_t mm;
    uint32_t odd;   // message on row 1 (else on row 0)
    int32_t aidx;   // automorphism key: index of its permuted secret (else -1)
    uint32_t pad;
};
static_assert(sizeof(KgRow) == 48, "descriptor layout");

// The descriptors of one key (p.timeopt ignored: the caller passes with_base(bg) per key of the map).
// sk [n] mod qKS; nullptr counts with the zero secret (the descriptor count does not depend on the secret).
void keygen_descriptors(const Params& p, const uint64_t* sk, uint64_t seed, std::vector<KgRow>& out);

// Cap on the A / [E, M] scratch of one chunk of row pairs (3 N u64 words per pair): 768 MiB, which is 32768 row
// pairs at N = 1024 (what the N = 1024 fast path uses) and 16384 at N = 2048.
constexpr size_t kKgScratchCap = (size_t)768 << 20;
inline size_t keygen_chunk_pairs(uint32_t N, size_t pairs) {
    const size_t cap = kKgScratchCap / ((size_t)3 * N * 8);
    return pairs < cap ? pairs : cap;
}
// device temporaries of one key's generation with `pairs` descriptors: the descriptors, S, the permuted secrets,
// one chunk of A / [E, M] and the switching key's vectors (sv, svN, digit powers)
size_t keygen_scratch_bytes(const Params& p, size_t pairs);

struct KeygenPlan {
    uint32_t on_device, keys;
    uint64_t row_pairs, ntt_polys, ksk_rows, scratch_bytes;
};
// What device BTKeyGen does for this set: filled by keygen_descriptors over every key of the map.
KeygenPlan keygen_plan(const Params& p);

}  // namespace fhe_amd
