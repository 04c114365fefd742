// nt.h -- host number theory for parameter setup (init only, never on the hot path).
// Restates the reference's LastPrime (src/core/include/math/nbtheory-impl.h:350-371),
// RootOfUnity (:183-228, minimal primitive root) and ReverseBits (nbtheory.h:135).
#pragma once
#include <stdint.h>

#include <vector>

namespace fhe_amd {

typedef unsigned __int128 u128;

inline uint64_t mulmod(uint64_t a, uint64_t b, uint64_t m) { return (uint64_t)(((u128)a * b) % m); }
inline uint64_t addmod(uint64_t a, uint64_t b, uint64_t m) { uint64_t s = a + b; return s >= m ? s - m : s; }
inline uint64_t submod(uint64_t a, uint64_t b, uint64_t m) { return a >= b ? a - b : a + m - b; }
uint64_t powmod(uint64_t b, uint64_t e, uint64_t m);
inline uint64_t invmod(uint64_t a, uint64_t m) { return powmod(a, m - 2, m); }  // m prime
bool is_prime(uint64_t n);
uint64_t last_prime(uint32_t bits, uint64_t m);
uint64_t root_of_unity(uint64_t m, uint64_t Q);
inline uint32_t reverse_bits(uint32_t x, uint32_t bits) {
    uint32_t r = 0;
    for (uint32_t i = 0; i < bits; ++i) r |= ((x >> i) & 1u) << (bits - 1 - i);
    return r;
}
inline uint32_t ilog2(uint64_t x) { uint32_t r = 0; while (x > 1) { x >>= 1; ++r; } return r; }
inline uint32_t shoup32(uint64_t w, uint64_t Q) { return (uint32_t)(((u128)w << 32) / Q); }
inline uint64_t shoup64(uint64_t w, uint64_t Q) { return (uint64_t)(((u128)w << 64) / Q); }
// the 32-bit kernels' Montgomery form x 2^32 mod Q and -Q^-1 mod 2^32 (Newton; Q odd: Q * Q = 1 mod 8)
inline uint32_t to_mont(uint64_t x, uint64_t Q) { return (uint32_t)(((u128)(x % Q) << 32) % Q); }
inline uint32_t neg_inv32(uint32_t Q) {
    uint32_t x = Q;
    for (int i = 0; i < 5; ++i) x *= 2 - Q * x;
    return (uint32_t)(0u - x);
}

// Constants of the signed forward passes' first 4-point group (bootstrap.hip fwd_group4): with I = Table[1],
// u = Table[2], v = Table[3] (plain residues mod an odd prime Q), the two stage-2 products of a group are
// u x + (I u) y and (I u) x + u y, a circulant, so they equal P + M and P - M with P = c+ (x + y),
// M = c- (x - y), c+- = (u +- I u) / 2.  That needs I^2 = -1 and v = +I u (what the bit-reversed power table
// gives: Table[3] = psi^(3N/4) = psi^(N/2) psi^(N/4)); v = -I u would swap the group's last two outputs, which
// the kernels do not implement.  False (and no constants) for any other table.
inline bool fwd_group_consts(uint64_t Q, uint64_t I, uint64_t u, uint64_t v, uint64_t* cp, uint64_t* cm) {
    if (Q < 3 || !(Q & 1) || I >= Q || u >= Q || v >= Q) return false;
    const uint64_t Iu = mulmod(I, u, Q);
    if (mulmod(I, I, Q) != Q - 1 || v != Iu) return false;
    const uint64_t half = (Q + 1) / 2;  // 2^-1 mod Q
    *cp = mulmod(addmod(u, Iu, Q), half, Q);
    *cm = mulmod(submod(u, Iu, Q), half, Q);
    return true;
}

// Product twiddles of two signed stages taken as one 4-point group (bootstrap.hip ct_group4_s / gs_group4_s).  The
// outer stage's twiddle w1 = Table[k] (k >= 2) goes with the inner stage's pair w2 = Table[2k], w3 = Table[2k + 1];
// the groups multiply by w1 w2 and by -(w1 w3) (returned in [0, Q)) instead of chaining two products.  In the
// bit-reversed power table Table[2k]^2 = Table[k] and Table[2k + 1] = Table[1] Table[2k] with Table[1]^2 = -1 (the
// same holds in TableI); the three are checked against each other and against I = Table[1] first, and the products
// against the cubes they must equal (w1 w2 = w2^3; w3^2 = -w1, so -(w1 w3) = w3^3).  False (and no products) for
// any other table.
inline bool stage_group_consts(uint64_t Q, uint64_t I, uint64_t w1, uint64_t w2, uint64_t w3, uint64_t* w12,
                               uint64_t* w13n) {
    if (Q < 3 || !(Q & 1) || I >= Q || w1 >= Q || w2 >= Q || w3 >= Q) return false;
    if (mulmod(I, I, Q) != Q - 1 || mulmod(w2, w2, Q) != w1 || mulmod(I, w2, Q) != w3) return false;
    const uint64_t p2 = mulmod(w1, w2, Q), p3n = submod(0, mulmod(w1, w3, Q), Q);
    if (p2 != mulmod(mulmod(w2, w2, Q), w2, Q) || p3n != mulmod(mulmod(w3, w3, Q), w3, Q)) return false;
    *w12  = p2;
    *w13n = p3n;
    return true;
}

// The product twiddles of one direction's grouped stage pairs, from that direction's bit-reversed table of
// N = 1024 (plain residues), as boot.h lays them out (kGroupUniWords + kGroupLaneWords entries):
//   out[2 j], out[2 j + 1], j < 4          the uniform pair on register bits 2 and 1 of layout A': Table[4 + j] with
//                                          Table[8 + 2 j], Table[9 + 2 j]
//   out[8 + 32 e + l], e < 10, l < 32      lane-major, layout B': e = 0, 1 the pair on bits 4 and 3 (Table[32 + l]
//                                          with Table[64 + 2 l], Table[65 + 2 l]); e = 2 + 2 j, 3 + 2 j the pair on
//                                          bits 2 and 1 (Table[128 + 4 l + j] with Table[256 + 8 l + 2 j], .. + 1)
// False as soon as one triple fails stage_group_consts.
inline bool stage_group_table(uint64_t Q, const uint64_t* tab, uint64_t* out) {
    for (int j = 0; j < 4; ++j)
        if (!stage_group_consts(Q, tab[1], tab[4 + j], tab[8 + 2 * j], tab[9 + 2 * j], &out[2 * j], &out[2 * j + 1]))
            return false;
    for (int l = 0; l < 32; ++l) {
        const int k = 32 + l;
        if (!stage_group_consts(Q, tab[1], tab[k], tab[2 * k], tab[2 * k + 1], &out[8 + l], &out[8 + 32 + l]))
            return false;
        for (int j = 0; j < 4; ++j) {
            const int kk = 128 + 4 * l + j;
            if (!stage_group_consts(Q, tab[1], tab[kk], tab[2 * kk], tab[2 * kk + 1], &out[8 + 32 * (2 + 2 * j) + l],
                                    &out[8 + 32 * (3 + 2 * j) + l]))
                return false;
        }
    }
    return true;
}

// Host NTT (same transform as the device kernels) for key generation.
struct HostNtt {
    uint32_t N = 0, logN = 0;
    uint64_t Q = 0, psi = 0, ninv = 0;
    std::vector<uint64_t> tab, tabI;  // Table[brv(i)] = psi^i, TableI[brv(i)] = psi^-i
    void init(uint32_t N, uint64_t Q, uint64_t psi);
    void forward(uint64_t* a) const;
    void inverse(uint64_t* a) const;
};

}  // namespace fhe_amd
