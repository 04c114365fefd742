// red_plan.h -- the compile-time reduction plan of the signed inverse transforms (bootstrap.hip inv_pass_s and
// inv_wave_s, boot_2k.h inv_2k_s, ntt.hip k_ntt1024w).  Plain constexpr C++17, no HIP: the kernels evaluate it at
// compile time, tests/red_plan_check.cpp runs it on the host.
//
// Gentleman-Sande on signed residues takes x' = x + y, y' = smont(x - y, w) in (-Q, Q): two adds and no reduction
// per butterfly.  Sums grow, and |x| + |y| must stay within the signed 32-bit range (LIM: 16 Q for Q < 2^27, 8 Q for
// Q < 2^28), so a register whose bound would pass it is brought back to (-Q, Q) first, by one signed Montgomery
// product with 2^32 mod Q.  Bounds are tracked per register in units of Q/10: within a layout every element a
// register holds has the same bound.  A transpose mixes every register, so the largest bound reaches all of them;
// registers above a threshold are reduced before it (without that the A stages of the LMKCDEY automorphism's
// inverse took 36 reductions per lane, with it 16).
#pragma once

#ifndef FHE_PLAN_T
#define FHE_PLAN_T 1  // 0: no reductions before the transposes of the searched plans (the round-4 plans)
#endif

namespace fhe_amd {

// Candidate thresholds (units of Q/10) red_plan_search tries before each transpose; the last is none
constexpr int kPlanT[8] = {10, 15, 20, 30, 40, 60, 80, 1 << 20};
constexpr int kPlanTN   = FHE_PLAN_T ? 8 : 0;
constexpr int kPlanNoT  = kPlanT[7];

// A shape: R registers, S stages in execution order, the register bit each stage pairs (the last stage pairs the
// top bit), and the stage each of up to two transposes precedes (-1: no such transpose).
// bootstrap.hip inv_pass_s: layout B' bits 0..4, the transpose, A' bits 0..3, the last stage
struct HalfWaveShape {
    static constexpr int R = 32, S = 10;
    static constexpr int bit[S] = {0, 1, 2, 3, 4, 0, 1, 2, 3, 4};
    static constexpr int tr[2]  = {5, -1};
};
// bootstrap.hip inv_wave_s, ntt.hip k_ntt1024w: C bits 0 and 1, C -> B, B bits 0..3, B -> A, A bits 0..2, the last
struct WaveShape {
    static constexpr int R = 16, S = 10;
    static constexpr int bit[S] = {0, 1, 0, 1, 2, 3, 0, 1, 2, 3};
    static constexpr int tr[2]  = {2, 6};
};
// boot_2k.h inv_2k_s (N = 2048): C bit 0, C -> B, B bits 0..4, B -> A, A bits 0..3, the last
struct N2kShape {
    static constexpr int R = 32, S = 11;
    static constexpr int bit[S] = {0, 0, 1, 2, 3, 4, 0, 1, 2, 3, 4};
    static constexpr int tr[2]  = {1, 6};
};

template <class Sh>
struct RedPlan {
    bool red[Sh::S][Sh::R];  // reduce register r before stage s
    bool redT[2][Sh::R];     // ... before transpose k
    int fin[Sh::R / 2];      // last-stage sum x + y: |.| < 2^fin Q -> add 2^fin Q, then fin + 1 conditional subtractions
    int cost;                // 2 per reduction + 1 per final conditional subtraction (their issue-cycle ratio)
    int T[2];                // the thresholds it was made with
};

// The plan from |v| < BIN Q / 10 under |x| + |y| <= LIM Q / 10, reducing registers above T0 / T1 before the transposes
template <class Sh>
constexpr RedPlan<Sh> red_plan(int BIN, int LIM, int T0, int T1) {
    static_assert((2 << Sh::bit[Sh::S - 1]) == Sh::R, "the last stage pairs the top bit: fin[r] is of (r, r | R / 2)");
    RedPlan<Sh> p{};
    p.T[0] = T0;
    p.T[1] = T1;
    int B[Sh::R] = {};
    for (int r = 0; r < Sh::R; ++r) B[r] = BIN;
    int nred = 0;
    for (int st = 0; st < Sh::S; ++st) {
        for (int k = 0; k < 2; ++k) {
            if (st != Sh::tr[k]) continue;
            int U = 0;
            for (int r = 0; r < Sh::R; ++r) {
                if (B[r] > p.T[k]) {
                    B[r]         = 10;
                    p.redT[k][r] = true;
                    ++nred;
                }
                U = B[r] > U ? B[r] : U;
            }
            for (int r = 0; r < Sh::R; ++r) B[r] = U;
        }
        const int bt = Sh::bit[st];
        for (int r = 0; r < Sh::R; ++r) {
            if (r & (1 << bt)) continue;
            const int q = r | (1 << bt);
            while (B[r] + B[q] > LIM) {
                const int e  = B[r] >= B[q] ? r : q;
                B[e]         = 10;
                p.red[st][e] = true;
                ++nred;
            }
            if (st == Sh::S - 1) {
                int f = 0;
                while ((10 << f) < B[r] + B[q]) ++f;
                p.fin[r] = f;
            }
            B[r] = B[r] + B[q];
            B[q] = 10;
        }
    }
    p.cost = 2 * nred;
    for (int r = 0; r < Sh::R / 2; ++r) p.cost += p.fin[r] + 1;
    return p;
}

// The cheapest plan over the candidate thresholds (the first of equal cost, the plan without thresholds first)
template <class Sh>
constexpr RedPlan<Sh> red_plan_search(int BIN, int LIM) {
    RedPlan<Sh> best = red_plan<Sh>(BIN, LIM, kPlanNoT, kPlanNoT);
    for (int a = 0; a < kPlanTN; ++a)
        for (int b = 0; b < kPlanTN; ++b) {
            const RedPlan<Sh> p = red_plan<Sh>(BIN, LIM, kPlanT[a], kPlanT[b]);
            if (p.cost < best.cost) best = p;
        }
    return best;
}

// The half-wave plan is not searched: it reduces what exceeds 2 Q before its one transpose
constexpr RedPlan<HalfWaveShape> red_plan_halfwave(int BIN, int LIM) {
    return red_plan<HalfWaveShape>(BIN, LIM, 20, kPlanNoT);
}

// Stage pairs as 4-point groups (bootstrap.hip gs_group4_s).  Stages st and st + 1 (register bits lo and hi, no
// transpose between them) on {a, b, c, d} = registers {r, r | lo, r | hi, r | lo | hi} give
//   a + b + c + d,   ((a + b) - (c + d)) w,   X u + Y v,   X u' - Y v'      (X = a - b, Y = c - d).
// The products X u and Y v of stage st are never formed, so stage st + 1 cannot reduce them, and the two-term
// outputs are below (|X| + |Y|) Q 2^-32 + Q/2 <= Q only for |X| + |Y| <= 2^31.  A mark of stage st + 1 never falls
// on the product registers r | lo and r | hi | lo (their pair is 10 + 10 <= LIM); one on r or r | hi means that
// |a| + |b| + |c| + |d| may pass LIM, and then |X| + |Y| may too.  So the plan is kept as it is (the same marks, the
// same bounds: a two-term output counts as 10 like a product) and a group is taken as one exactly when stage
// st + 1 marks none of its registers -- then LIM Q / 10 <= 2^31 bounds |X| + |Y| as well; the others run their
// two stages apart.  Not built: a planner of its own for the grouped shape, which resets inputs until every group
// qualifies and counts a two-term output as 10 where this one counts 10 + 10.  From 2.8 Q and LIM 16 Q it places 22
// resets instead of 19 and takes all 24 groups of the three inverse pairs instead of 19, 6 instructions fewer
// in all (tests/red_plan_groups_check.cpp prints both); for the pair the kernels take (A' bits 1, 2: every group
// admitted as it is) the two are the same.
template <class Sh>
constexpr bool red_plan_group_ok(const RedPlan<Sh>& p, int st, int r) {
    const int lo = 1 << Sh::bit[st], hi = 1 << Sh::bit[st + 1];
    const bool(&row)[Sh::R] = p.red[st + 1];
    return !row[r] && !row[r | lo] && !row[r | hi] && !row[r | lo | hi];
}
// The largest |X| + |Y| (units of Q / 10) over the two-term legs of the groups of stages st, st + 1 that
// red_plan_group_ok admits, and the number of those groups, by replaying the plan's bounds from BIN; -1 if a
// butterfly's |x| + |y| passes LIM anywhere in the replay (a plan made for other inputs)
template <class Sh>
constexpr int red_plan_group_legs(const RedPlan<Sh>& p, int BIN, int LIM, int st, int* groups) {
    int B[Sh::R] = {};
    for (int r = 0; r < Sh::R; ++r) B[r] = BIN;
    int worst = 0, n = 0;
    for (int s = 0; s < Sh::S; ++s) {
        for (int k = 0; k < 2; ++k) {
            if (s != Sh::tr[k]) continue;
            int U = 0;
            for (int r = 0; r < Sh::R; ++r) {
                if (p.redT[k][r]) B[r] = 10;
                U = B[r] > U ? B[r] : U;
            }
            for (int r = 0; r < Sh::R; ++r) B[r] = U;
        }
        const int bt = 1 << Sh::bit[s];
        for (int r = 0; r < Sh::R; ++r)
            if (p.red[s][r]) B[r] = 10;
        if (s == st) {
            const int hi = 1 << Sh::bit[st + 1];
            for (int r = 0; r < Sh::R; ++r) {
                if ((r & bt) || (r & hi) || !red_plan_group_ok(p, st, r)) continue;
                const int legs = B[r] + B[r | bt] + B[r | hi] + B[r | bt | hi];
                worst = legs > worst ? legs : worst;
                ++n;
            }
        }
        for (int r = 0; r < Sh::R; ++r) {
            if (r & bt) continue;
            if (B[r] + B[r | bt] > LIM) return -1;
            B[r] += B[r | bt];
            B[r | bt] = 10;
        }
    }
    if (groups) *groups = n;
    return worst;
}

}  // namespace fhe_amd
