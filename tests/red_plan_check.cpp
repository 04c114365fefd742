// Prints the reduction plans of fhe_amd/csrc/red_plan.h as text; tests/test_red_plan.py does the checking.
//   red_plan_check grid    every BIN 10..120 x LIM {40, 80, 160} x the three shapes and the ntt.hip point, with the
//                          thresholds used and, for the searched shapes, the cost of each of the 65 candidates
//   red_plan_check golden  the points of tests/golden/red_plans.txt, tables only
#include <cstdio>
#include <cstring>

#include "red_plan.h"

using namespace fhe_amd;

template <class Sh>
static void print_shape(const char* name) {
    std::printf("shape %s R %d S %d bits", name, Sh::R, Sh::S);
    for (int s = 0; s < Sh::S; ++s) std::printf(" %d", Sh::bit[s]);
    std::printf(" tr %d %d\n", Sh::tr[0], Sh::tr[1]);
}

template <int R>
static unsigned mask(const bool (&row)[R]) {
    unsigned m = 0;
    for (int r = 0; r < R; ++r) m |= (unsigned)row[r] << r;
    return m;
}

template <class Sh>
static void print_plan(const char* name, int BIN, int LIM, const RedPlan<Sh>& p, bool thresholds) {
    std::printf("plan %s BIN %d LIM %d\n", name, BIN, LIM);
    if (thresholds) std::printf("T %d %d\n", p.T[0], p.T[1]);
    std::printf("red");
    for (int s = 0; s < Sh::S; ++s) std::printf(" %08x", mask(p.red[s]));
    std::printf("\nredT %08x %08x\nfin", mask(p.redT[0]), mask(p.redT[1]));
    for (int r = 0; r < Sh::R / 2; ++r) std::printf(" %d", p.fin[r]);
    std::printf("\ncost %d\n", p.cost);
}

template <class Sh>
static void print_costs(int BIN, int LIM) {
    std::printf("costs %d", red_plan<Sh>(BIN, LIM, kPlanNoT, kPlanNoT).cost);
    for (int a = 0; a < 8; ++a)
        for (int b = 0; b < 8; ++b) std::printf(" %d", red_plan<Sh>(BIN, LIM, kPlanT[a], kPlanT[b]).cost);
    std::printf("\n");
}

static void point(int BIN, int LIM, bool grid) {
    print_plan("half", BIN, LIM, red_plan_halfwave(BIN, LIM), grid);
    print_plan("wave", BIN, LIM, red_plan_search<WaveShape>(BIN, LIM), grid);
    if (grid) print_costs<WaveShape>(BIN, LIM);
    print_plan("n2k", BIN, LIM, red_plan_search<N2kShape>(BIN, LIM), grid);
    if (grid) print_costs<N2kShape>(BIN, LIM);
}

int main(int argc, char** argv) {
    const int lims[3] = {40, 80, 160};
    if (argc == 2 && !std::strcmp(argv[1], "grid")) {
        print_shape<HalfWaveShape>("half");
        print_shape<WaveShape>("wave");
        print_shape<N2kShape>("n2k");
        std::printf("thresholds");
        for (int t : kPlanT) std::printf(" %d", t);
        std::printf("\n");
        for (int LIM : lims)
            for (int BIN = 10; BIN <= 120; ++BIN) point(BIN, LIM, true);
        print_plan("ntt", 10, 160, red_plan<WaveShape>(10, 160, kPlanNoT, kPlanNoT), true);
        return 0;
    }
    if (argc == 2 && !std::strcmp(argv[1], "golden")) {
        const int bins[16] = {10, 20, 22, 24, 25, 27, 28, 29, 30, 32, 33, 36, 37, 39, 53, 105};
        for (int LIM : lims)
            for (int BIN : bins) point(BIN, LIM, false);
        return 0;
    }
    std::fprintf(stderr, "usage: red_plan_check grid|golden\n");
    return 2;
}
