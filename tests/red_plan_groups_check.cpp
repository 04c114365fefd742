// Replays the half-wave reduction plan of fhe_amd/csrc/red_plan.h with the stage pairs K1 takes as 4-point groups
// (red_plan_group_ok), from worst-case bounds, for the BIN / LIM points the kernels use; tests/test_k1_stage_groups.py
// compiles and runs it.  Bounds are per register in units of Q / 10, as the plan keeps them; LIM Q / 10 <= 2^31.
//   - every butterfly and every group sum keeps |x| + |y| <= LIM;
//   - every two-term leg of an admitted group has |X| + |Y| <= LIM, hence <= 2^31;
//   - an admitted group's product outputs count as 10 (below Q), as the plan assumes for the two stages apart.
// Prints, per point and pair, the admitted groups of 8 and the largest |X| + |Y|; then the plan's reset count (the same
// with and without groups: a group that would need another mark runs as two stages) next to that of a planner that
// resets inputs until every group is taken, each with its instruction cost.  Exit status 1 on a violated bound.
#include <cstdio>

#include "red_plan.h"

using namespace fhe_amd;
using Sh = HalfWaveShape;

static int reductions(const RedPlan<Sh>& p) {
    int n = 0;
    for (int r = 0; r < Sh::R; ++r) {
        for (int s = 0; s < Sh::S; ++s) n += p.red[s][r];
        n += p.redT[0][r];
    }
    return n;
}

// the replay with groups at the first stages in `firsts` (stage indices, -1 terminated)
static bool replay(const RedPlan<Sh>& p, int BIN, int LIM, const int* firsts, int* admitted, int* worst_legs) {
    int B[Sh::R];
    for (int r = 0; r < Sh::R; ++r) B[r] = BIN;
    bool ok = true;
    for (int s = 0; s < Sh::S; ++s) {
        if (s == Sh::tr[0]) {
            int U = 0;
            for (int r = 0; r < Sh::R; ++r) {
                if (p.redT[0][r]) B[r] = 10;
                U = B[r] > U ? B[r] : U;
            }
            for (int r = 0; r < Sh::R; ++r) B[r] = U;
        }
        int gi = -1;
        for (int k = 0; firsts[k] >= 0; ++k)
            if (firsts[k] == s) gi = k;
        bool second = false;
        for (int k = 0; firsts[k] >= 0; ++k) second |= firsts[k] + 1 == s;
        const int bt = 1 << Sh::bit[s];
        for (int r = 0; r < Sh::R; ++r) {
            if (r & bt) continue;
            const int q = r | bt;
            if (second && red_plan_group_ok(p, s - 1, r & ~(1 << Sh::bit[s - 1]))) continue;  // done with stage s - 1
            if (gi >= 0) {
                const int hi = 1 << Sh::bit[s + 1], base = r & ~hi;
                if (red_plan_group_ok(p, s, base)) {
                    if (r & hi) continue;
                    const int g[4] = {r, q, r | hi, q | hi};
                    for (int x : g)
                        if (p.red[s][x]) B[x] = 10;
                    const int X = B[g[0]] + B[g[1]], Y = B[g[2]] + B[g[3]];
                    if (X > LIM || Y > LIM || X + Y > LIM) {
                        std::printf("VIOLATION stage %d group %d: |X| %d |Y| %d LIM %d\n", s, r, X, Y, LIM);
                        ok = false;
                    }
                    ++admitted[gi];
                    worst_legs[gi] = X + Y > worst_legs[gi] ? X + Y : worst_legs[gi];
                    B[g[0]] = X + Y;  // a + b + c + d
                    B[g[1]] = 10;     // two-term leg: (X + Y) Q 2^-32 + Q / 2 <= Q for X + Y <= 2^31
                    B[g[2]] = 10;     // one product
                    B[g[3]] = 10;     // two-term leg
                    continue;
                }
            }
            if (p.red[s][r]) B[r] = 10;
            if (p.red[s][q]) B[q] = 10;
            if (B[r] + B[q] > LIM) {
                std::printf("VIOLATION stage %d pair %d: %d + %d > LIM %d\n", s, r, B[r], B[q], LIM);
                ok = false;
            }
            B[r] += B[q];
            B[q] = 10;
        }
    }
    return ok;
}

// The alternative to running a marked group as two stages: a planner that resets a group's largest inputs until
// |a| + |b| + |c| + |d| <= LIM, so that every group of the pairs in `firsts` is taken as one; elsewhere the rule of
// red_plan (reset the larger of a pair that would pass LIM; what exceeds 2 Q before the transpose).  Returns its
// number of resets.
static int alt_resets(int BIN, int LIM, const int* firsts) {
    int B[Sh::R], n = 0;
    for (int r = 0; r < Sh::R; ++r) B[r] = BIN;
    for (int s = 0; s < Sh::S; ++s) {
        if (s == Sh::tr[0]) {
            int U = 0;
            for (int r = 0; r < Sh::R; ++r) {
                if (B[r] > 20) B[r] = 10, ++n;
                U = B[r] > U ? B[r] : U;
            }
            for (int r = 0; r < Sh::R; ++r) B[r] = U;
        }
        bool first = false, second = false;
        for (int k = 0; firsts[k] >= 0; ++k) first |= firsts[k] == s, second |= firsts[k] + 1 == s;
        if (second) continue;
        const int bt = 1 << Sh::bit[s];
        for (int r = 0; r < Sh::R; ++r) {
            if (r & bt) continue;
            const int q = r | bt;
            if (first) {
                const int hi = 1 << Sh::bit[s + 1];
                if (r & hi) continue;
                const int g[4] = {r, q, r | hi, q | hi};
                for (;;) {
                    int sum = 0, big = 0;
                    for (int i = 0; i < 4; ++i) {
                        sum += B[g[i]];
                        if (B[g[i]] > B[g[big]]) big = i;
                    }
                    if (sum <= LIM) break;
                    B[g[big]] = 10, ++n;
                }
                B[g[0]] = B[g[0]] + B[g[1]] + B[g[2]] + B[g[3]];
                B[g[1]] = B[g[2]] = B[g[3]] = 10;
                continue;
            }
            while (B[r] + B[q] > LIM) B[B[r] >= B[q] ? r : q] = 10, ++n;
            B[r] += B[q];
            B[q] = 10;
        }
    }
    return n;
}

int main() {
    // K1 GINX (Q < 2^27, |acc| < 2.8 Q), the LMKCDEY / AP op-list kernel (2 Q for Q < 2^27; 2.4 Q for Q < 2^28)
    const int points[3][2] = {{28, 160}, {20, 160}, {24, 80}};
    const int firsts[4] = {1, 3, 6, -1};
    const char* names[3] = {"B' bits 1,2", "B' bits 3,4", "A' bits 1,2"};
    bool ok = true;
    for (const auto& pt : points) {
        const int BIN = pt[0], LIM = pt[1];
        if ((long long)LIM * (1 << 28) / (LIM == 160 ? 2 : 1) / 10 > (1LL << 31)) ok = false;  // LIM Q / 10 <= 2^31
        const RedPlan<Sh> p = red_plan_halfwave(BIN, LIM);
        int admitted[3] = {}, legs[3] = {};
        ok &= replay(p, BIN, LIM, firsts, admitted, legs);
        const int none[1] = {-1};
        int a0[1] = {}, l0[1] = {};
        ok &= replay(p, BIN, LIM, none, a0, l0);
        for (int k = 0; k < 3; ++k) {
            int n = 0;
            const int w = red_plan_group_legs(p, BIN, LIM, firsts[k], &n);
            // the plan's own accounting (a group's second output as 10 + 10, as two stages apart) bounds the replay's
            if (w < 0 || w < legs[k] || n != admitted[k] || w > LIM) {
                std::printf("VIOLATION red_plan_group_legs stage %d: %d / %d groups, legs %d / %d\n", firsts[k], n,
                            admitted[k], w, legs[k]);
                ok = false;
            }
            std::printf("BIN %d LIM %d %s: %d of 8 groups, largest |X| + |Y| %d (Q / 10), saves %d instructions\n", BIN,
                        LIM, names[k], admitted[k], legs[k], 3 * admitted[k]);
        }
        // instructions over the grouped form with no reset at all: 3 per reset, 3 per group run as two stages
        const int groups = admitted[0] + admitted[1] + admitted[2], alt = alt_resets(BIN, LIM, firsts);
        const int cost_fallback = 3 * reductions(p) + 3 * (24 - groups), cost_alt = 3 * alt;
        std::printf("BIN %d LIM %d resets: %d in the plan (without groups, and with %d of 24 groups taken: %d instructions), "
                    "%d with inputs reset until all 24 are taken (%d instructions)\n",
                    BIN, LIM, reductions(p), groups, cost_fallback, alt, cost_alt);
    }
    std::printf(ok ? "OK\n" : "FAILED\n");
    return ok ? 0 : 1;
}
