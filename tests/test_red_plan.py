"""The compile-time reduction plans of the signed inverse transforms (fhe_amd/csrc/red_plan.h), checked on the host.

tests/red_plan_check.cpp prints the plans the planner makes (plain host code, built with ASan and UBSan); the checks
are here, so the checker is not the code under test:
  1. soundness: every printed plan is replayed in exact integers (units of Q/10) -- no butterfly's |x| + |y| passes
     LIM, fin is the least width of the last sums, cost is what the plan says it counts;
  2. the search returns the cheapest of its 65 candidates;
  3. the tables of every (BIN, LIM) the kernels instantiate equal tests/golden/red_plans.txt, written from the four
     hand-written planners this one replaced (profiles/red_plan_parent_compare.txt).
CPU-only: no GPU and no library load."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name: (registers, the register bit of each stage, the stage each transpose precedes)
SHAPES = {
    "half": (32, [0, 1, 2, 3, 4, 0, 1, 2, 3, 4], [5, -1]),
    "wave": (16, [0, 1, 0, 1, 2, 3, 0, 1, 2, 3], [2, 6]),
    "n2k": (32, [0, 0, 1, 2, 3, 4, 0, 1, 2, 3, 4], [1, 6]),
}
SHAPES["ntt"] = SHAPES["wave"]
PLAN_T = [10, 15, 20, 30, 40, 60, 80, 1 << 20]
NONE = PLAN_T[-1]
LIMS = (40, 80, 160)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("red_plan") / "red_plan_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "fhe_amd", "csrc"),
                            os.path.join(ROOT, "tests", "red_plan_check.cpp"), "-o", out],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    return out


def run(exe, mode):
    r = subprocess.run([exe, mode], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stderr
    return r.stdout


@pytest.fixture(scope="module")
def grid(exe):
    """(shape lines, thresholds, plans) of the grid run; a plan is a dict of its printed fields"""
    shapes, thresholds, plans = {}, None, []
    for ln in run(exe, "grid").splitlines():
        w = ln.split()
        if w[0] == "shape":
            assert w[2] == "R" and w[4] == "S" and w[6] == "bits" and w[-3] == "tr"
            shapes[w[1]] = (int(w[3]), [int(x) for x in w[7:-3]], [int(w[-2]), int(w[-1])])
            assert int(w[5]) == len(shapes[w[1]][1])
        elif w[0] == "thresholds":
            thresholds = [int(x) for x in w[1:]]
        elif w[0] == "plan":
            assert w[2] == "BIN" and w[4] == "LIM"
            plans.append({"shape": w[1], "BIN": int(w[3]), "LIM": int(w[5])})
        elif w[0] in ("red", "redT"):
            plans[-1][w[0]] = [int(x, 16) for x in w[1:]]
        elif w[0] in ("T", "fin", "costs"):
            plans[-1][w[0]] = [int(x) for x in w[1:]]
        else:
            assert w[0] == "cost", ln
            plans[-1]["cost"] = int(w[1])
    return shapes, thresholds, plans


def test_shapes_and_scope(grid):
    shapes, thresholds, plans = grid
    assert shapes == {k: v for k, v in SHAPES.items() if k != "ntt"}
    assert thresholds == PLAN_T
    want = [(s, b, lim) for lim in LIMS for b in range(10, 121) for s in ("half", "wave", "n2k")] + [("ntt", 10, 160)]
    assert [(p["shape"], p["BIN"], p["LIM"]) for p in plans] == want
    for p in plans:
        if p["shape"] == "half":
            assert p["T"] == [20, NONE]  # fixed: 2 Q before its one transpose
        elif p["shape"] == "ntt":
            assert p["T"] == [NONE, NONE]
        else:
            assert p["T"][0] in PLAN_T and p["T"][1] in PLAN_T


def marked(mask, R):
    assert mask >> R == 0
    return [r for r in range(R) if mask >> r & 1]


def replay(p):
    """the plan applied to bounds that start at BIN: asserts its soundness, its fin and its cost"""
    R, bits, tr = SHAPES[p["shape"]]
    LIM, last = p["LIM"], len(bits) - 1
    assert len(p["red"]) == len(bits) and len(p["redT"]) == 2 and len(p["fin"]) == R // 2
    B = [p["BIN"]] * R
    marks = 0
    for st, bt in enumerate(bits):
        for k in (0, 1):
            if tr[k] < 0:
                assert p["redT"][k] == 0
            if st == tr[k]:
                for r in marked(p["redT"][k], R):
                    B[r] = 10
                    marks += 1
                B = [max(B)] * R
        for r in marked(p["red"][st], R):
            B[r] = 10
            marks += 1
        for r in range(R):
            if r & (1 << bt):
                continue
            q = r | (1 << bt)
            assert B[r] + B[q] <= LIM, (p["shape"], p["BIN"], LIM, st, r)
            if st == last:
                f = p["fin"][r]
                assert 10 << f >= B[r] + B[q], (p["shape"], p["BIN"], LIM, r)
                assert f == 0 or 10 << (f - 1) < B[r] + B[q], (p["shape"], p["BIN"], LIM, r)
            B[r] += B[q]
            B[q] = 10
    assert p["cost"] == 2 * marks + sum(f + 1 for f in p["fin"]), (p["shape"], p["BIN"], LIM)


def test_soundness_replay(grid):
    for p in grid[2]:
        replay(p)


def test_search_returns_the_cheapest(grid):
    searched = [p for p in grid[2] if p["shape"] in ("wave", "n2k")]
    assert len(searched) == 2 * 3 * 111
    for p in searched:
        costs = p["costs"]  # the plan without thresholds, then kPlanT[a] x kPlanT[b]
        assert len(costs) == 65
        assert p["cost"] == min(costs), (p["shape"], p["BIN"], p["LIM"])
        assert costs[1 + 8 * PLAN_T.index(p["T"][0]) + PLAN_T.index(p["T"][1])] == p["cost"]
    assert all("costs" not in p for p in grid[2] if p["shape"] in ("half", "ntt"))


def test_pinned_to_the_replaced_planners(exe):
    golden = open(os.path.join(ROOT, "tests", "golden", "red_plans.txt")).read()
    assert golden.count("plan ") == 144
    assert run(exe, "golden") == golden
