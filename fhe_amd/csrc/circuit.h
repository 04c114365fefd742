// circuit.h -- circuits over the gate and functional bootstraps: the DAG a caller builds, its level plan (host
// only, no device or context), and the per-node descriptors the indexed prep and linear kernels read.
//
// The counterpart of the reference's BatchDAG (src/binfhe/include/batch/binfhe-batch.h:229-279), whose
// Execute runs one gate at a time (src/binfhe/lib/batch/batch.cpp:429-482).  Here every level of the DAG
// is a few launch classes, each one prep + blind rotation + key switch over all of its slots
// (DESIGN.md §4 "Circuits"):
//   class 0  gates of any 2-input types, BOOTSTRAP nodes and the multi-input gates at plaintext modulus 4, in
//            AND's window,
//   class 1  test-vector tables at ciphertext modulus q (FUNC nodes with negacyclic and periodic LUTs),
//   class 2  tables at 2q (FUNC nodes with arbitrary LUTs),
//   one more gate class per plaintext modulus other than 4 that the level's multi-input gates use, in ascending
//   order of the modulus: AND's window again, with the values Q/(2p) + 1 of that modulus,
// followed by one element-wise launch for the level's LINEAR nodes (no bootstrap).
//
// MULTI(gate, xs[k], p), gate one of MAJORITY / AND3 / OR3 / AND4 / OR4 and 2 <= k <= 4, is EvalBinGate(gate,
// ctvector) (binfhe-base-scheme.cpp:127-170) at plaintext modulus p: one bootstrap of the sum of its operands.
// BootstrapGateCore gives every gate the half-circle window [q1, q1 + q/2) (:535-553), so bshift = q1(AND) - q1(gate)
// folds it onto AND's window as it does for the 2-input gates; what differs between plaintext moduli is the value
// Q/(2p) + 1 the accumulator kernels take per launch, hence the class per modulus.  At p = 4 that value is AND's,
// and MAJORITY's window is AND's: a MAJORITY node is a class-0 slot with three operands and bshift = 0.  An
// operand may be any node; a NOT alias folds in as a sign flip and q/4, as for 2-input gates.  The circuit does
// not type-check encodings (the reference takes p from ctvector[0]): the caller owns the plaintext modulus of what
// it wires together, and only p = 4 nodes compose with 2-input gates and NOT.  The number of distinct moduli in
// a circuit or a level is not capped.
//
// FUNC(x, lut) is EvalFunc (binfhe-base-scheme.cpp:241-337), expanded by the plan into the one or two
// bootstraps Engine::eval_func_device sequences; its class (checkInputFunction) is fixed when the node is added.
// Its operand must not resolve to a NOT alias: EvalNOT's (-a, q/4 - b) is a negation mod q, which is no
// negation of the same ciphertext once an arbitrary LUT lifts it to 2q, so such an operand is refused for
// every class (bootstrap it, or fold the NOT into the LUT).  lut's length must equal the parameter set's q,
// which is only known at evaluation: a mismatch is refused there, as is the arbitrary class when q > N (the
// reference's own condition) or under AP (its accumulator reads a mod q only).
// LINEAR(xs[k], signs[k], c), 1 <= k <= 4, is sum_j +-x_j + (0, c mod q) mod q (EvalAddEq / EvalSubEq /
// EvalAddConstEq, lwe-pke.cpp:230-246) in a pool row of its own, at the highest level of its operands.  A NOT
// alias operand folds in as a sign flip and +-q/4; a LINEAR operand is refused (the caller flattens it).
//
// Not supported, refused when the node is added (std::invalid_argument, FHE_HIP_ERR_INVALID_PARAM):
//   - inputs mod Q (every input is a ciphertext mod q of dimension n),
//   - more than 65535 tables in one class (the table index is 16 bits of the prep's output word).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <map>
#include <utility>
#include <vector>

#include "params.h"

namespace fhe_amd {

// The ciphertext one slot of a level launch bootstraps (bootstrap.hip PoolFetch):
//   ct = sum_{j < k} (-1)^{neg_j} pool[src_j B + inst] + (0, boff_pre) mod ctmod, doubled when dbl, then b += bshift.
// ctmod is the launch's: q for gates and class-1 tables, 2q for class-2 tables (operands mod q are lifted
// with their values unchanged, binfhe-base-scheme.cpp:278-281).
// boff_pre: q/4 per negated operand (EvalNOT, binfhe-base-scheme.cpp:223-236) plus q/4 for BOOTSTRAP (:201);
// table slots: EvalFunc's beta, and - q/4 (periodic) or - q/2 (arbitrary) in its second stage (:292-294, :319-321).
// bshift = q1(AND) - q1(gate) mod q moves the gate's window onto the level's one launch window (AND's).
// Table slots carry their table's index within the class in the high half of flags; the prep hands it to the
// accumulator kernels in the high half of its b word (tvb).
struct CircuitSlot {
    uint32_t src[4];  // pool rows of the operands; k = 1: src[1] = src[0], k = 3: src[3] = src[2] (fetched, not
                      // used: PoolFetch reads rows in pairs), src[2..3] = 0 for k <= 2 (not fetched)
    uint32_t k;       // 1 (BOOTSTRAP, x + beta of a FUNC) .. 4; 2-input gates and FUNC second stages: 2
    uint32_t flags;   // kNeg << j: operand j is subtracted
    uint32_t boff_pre, bshift;
    static constexpr uint32_t kDbl = 4, kNeg = 0x100, kTableMask = 0xffff0000u, kTableShift = 16;
};
static_assert(sizeof(CircuitSlot) == 32, "CircuitSlot is read as two 16-byte words");

// A LINEAR row (circuit_gather.hip k_circuit_linear): sum_{j < k} (-1)^{neg_mask bit j} pool[src_j B + inst] + (0, c) mod q
struct CircuitLinear {
    uint32_t src[4];
    uint32_t k, neg_mask, c, pad;
};

// checkInputFunction (binfhe-base-scheme.h:245-260) of a LUT over Z_mod: 0 negacyclic, 1 periodic, 2 arbitrary
int lut_property(const uint64_t* lut, uint64_t len, uint64_t mod);
// test-vector functions f(x, q = ctmod, Q = fmod) of the reference's lambdas (fb.cpp, circuit.cpp)
enum TvKind { TV_LUT, TV_LUT_ANTI, TV_HALF, TV_FLOOR2, TV_SIGN, TV_SIGN_SS };
std::vector<uint64_t> tv_values(TvKind kind, const uint64_t* lut, uint64_t lutlen, uint64_t q, uint64_t fmod);

// An output row: pool row src, EvalNOT applied when neg
struct CircuitOut {
    uint32_t src, neg;
};

// q1(gate), the XOR / XNOR doubling and bshift = q1(ref) - q1(gate) mod q for two 2-input gates
// (OR, AND, NOR, NAND, XOR, XNOR, XOR_FAST, XNOR_FAST); std::invalid_argument for any other code
struct GateFold {
    uint32_t dbl, bshift, q1;
};
GateFold gate_fold(const Params& p, int gate, int ref_gate);

// BootstrapGateCore's window of any gate but CMUX at plaintext modulus ptmod (binfhe-base-scheme.cpp:535-556): its
// start q1, the value Q/(2 ptmod) + 1 the test vector holds (+-), the b the extraction adds (Q/(2 ptmod) + 1 for
// the multi-input gates, :162; (Q >> 3) + 1 for the 2-input ones whatever ptmod, :118) and q1(AND) - q1 mod q.
// std::invalid_argument for CMUX or an unknown code, ptmod < 2 or 2 ptmod > q.
struct GateWindow {
    uint64_t q1, value, b_const, bshift_to_and;
};
GateWindow gate_window(const Params& p, int gate, uint32_t ptmod);

class Circuit {
public:
    // Nodes get consecutive ids from 0 in the order they are added; operands must be existing ids, so the
    // graph is acyclic by construction.  Every add throws std::invalid_argument on an unknown id, an
    // unsupported gate code, GATE(g, x, x) on one (node, negation) pair (the reference's ct1 == ct2
    // check, binfhe-base-scheme.cpp:85-86; AND(x, NOT x) is two different ciphertexts and is accepted),
    // or a circuit that is already finalized.  Queries of the plan and evaluation throw std::logic_error
    // before finalize().
    uint32_t add_input();
    uint32_t add_not(uint32_t x);                                // no bootstrap: an alias (node, negated)
    uint32_t add_gate(int gate, uint32_t x, uint32_t y);
    // EvalBinGate(gate, ctvector) for MAJORITY / AND3 / OR3 / AND4 / OR4 over 2 <= k <= 4 operands (the rule of
    // Engine::eval_gate_multi_device) at plaintext modulus ptmod >= 2.  Refused: any other gate code, k out of
    // range, two operands on one (node, negation) pair (the reference's pairwise check, :136-143;
    // MAJORITY(x, NOT x, y) is three different ciphertexts).  2 ptmod > q is refused by check_params.
    uint32_t add_gate_multi(int gate, const uint32_t* xs, size_t k, uint32_t ptmod);
    uint32_t add_cmux(uint32_t c0, uint32_t c1, uint32_t sel);   // sel ? c1 : c0, as Engine::cmux_levels folds it
    uint32_t add_bootstrap(uint32_t x);                          // BinFHEScheme::Bootstrap
    // EvalFunc(x, lut): len a power of two >= 4, every value < len; x not a NOT alias (header comment)
    uint32_t add_func(uint32_t x, const uint64_t* lut, size_t len);
    // sum_j (signs[j] < 0 ? -1 : 1) xs[j] + (0, c); signs == nullptr: all +; no operand may be a LINEAR node
    uint32_t add_linear(const uint32_t* xs, const int* signs, size_t k, uint64_t c);
    void mark_output(uint32_t id);
    // Expands CMUX into its three NANDs, levelises (inputs level 0, a bootstrapped node 1 + its operands'
    // highest level, NOT the level of its source) and numbers the pool rows: inputs first, then level by
    // level, so each level's outputs are one contiguous block of rows.
    void finalize();
    bool finalized() const { return finalized_; }
    // unique per finalized circuit in this process (0 before): what a context's descriptor cache is keyed by
    uint64_t serial() const { return serial_; }
    // slots (gates x instances) per launch: 0 = the context's max_batch(); smaller values cut a level into
    // contiguous chunks
    void set_max_slots(size_t m) { max_slots_ = m; }
    size_t max_slots() const { return max_slots_; }

    size_t num_nodes() const { return nodes_.size(); }
    size_t num_inputs() const { return n_in_; }
    size_t num_outputs() const { return outs_.size(); }
    // after finalize()
    size_t num_levels() const { return level_row_.empty() ? 0 : level_row_.size() - 2; }  // bootstrapped levels
    size_t level_width(size_t level) const;   // level 0: the inputs
    size_t level_row(size_t level) const;     // first pool row of the level
    size_t num_bootstraps() const { return slots_.size(); }
    size_t num_linears() const { return lins_.size(); }
    size_t num_rows() const { return phys_.size(); }
    void node_row(uint32_t id, uint32_t* row, uint32_t* neg) const;
    // 0 negacyclic, 1 periodic, 2 arbitrary for a FUNC node, -1 for any other (known when the node is added)
    int func_class(uint32_t id) const;
    // A level's rows, in row order: w[0..2] the bootstraps of launch classes 0..2 (each one contiguous block;
    // within class 2 the first stages come first), w[3] its LINEAR rows.  Level 0: inputs are not counted.
    // w[0] includes the multi-input gates at plaintext modulus 4.  The gate classes of the other plaintext moduli
    // lie between class 2 and the LINEAR rows and are not in w: level_gate_classes.
    void level_classes(size_t level, size_t w[4]) const;
    // the level's (plaintext modulus, width) pairs of those extra gate classes, in row order (ascending modulus)
    const std::vector<std::pair<uint32_t, size_t>>& level_gate_classes(size_t level) const;
    size_t level_arb_stage1(size_t level) const;  // first-stage slots at the head of the level's class 2
    size_t level_slot(size_t level) const;        // index in slots() of the level's first bootstrap
    size_t level_linear(size_t level) const;      // index in linears() of the level's first LINEAR row
    // Descriptors of the bootstrapped rows in pool-row order for a parameter set: gate codes, negations and
    // the fold constants of gate_fold(p, gate, AND); table slots per the expansion above.  A circuit without
    // LINEAR nodes has slot i writing row num_inputs() + i.
    std::vector<CircuitSlot> slots(const Params& p) const;
    std::vector<CircuitLinear> linears(const Params& p) const;
    std::vector<CircuitOut> outputs() const;
    // Tables of launch class cls (1 or 2) for a parameter set: num_tables(cls) tables of table_ctmod(p, cls)
    // words, (Q / fmod) f(x) with fmod = ctmod (BootstrapFuncCore, binfhe-base-scheme.cpp:596-608).
    // std::invalid_argument when a LUT's length is not q, or for class 2 when q > N or the method is AP.
    size_t num_tables(int cls) const;
    static uint32_t table_ctmod(const Params& p, int cls) { return cls == 2 ? 2 * p.q : p.q; }
    std::vector<uint64_t> tables(const Params& p, int cls) const;
    // the refusals of tables(), for both classes, and a multi-input gate's plaintext modulus with 2 ptmod > q
    void check_params(const Params& p) const;

private:
    enum Kind : uint8_t { K_INPUT, K_NOT, K_GATE, K_CMUX, K_BOOTSTRAP, K_FUNC, K_LINEAR, K_MULTI };
    struct Node {
        Kind kind;
        int gate;
        uint32_t in[3];
    };
    struct Ref {  // a bootstrapped node or input, possibly negated
        uint32_t phys, neg;
    };
    // an input (gate = kInput), one bootstrap: a 2-input gate, BOOTSTRAP (gate = kBoot), a table slot (gate =
    // kTable: launch class cls, stage 1 or 2 of EvalFunc, aux = its table in the class; y = the first stage's
    // row in stage 2 of a two-stage class) or a multi-input gate (k operands x, y, z[0], z[1]; ptmod), or a
    // LINEAR row (gate = kLinear, aux = index in lin_)
    struct Phys {
        int gate;
        Ref x, y;
        uint32_t level, row;
        uint8_t cls, stage;
        uint32_t aux;
        Ref z[2];
        uint32_t k, ptmod;  // ptmod: 0 for everything but a multi-input gate
    };
    struct Lin {
        Ref x[4];
        uint32_t k;
        uint64_t c;
    };
    struct TableSpec {
        TvKind kind;
        uint32_t lut;  // index in luts_ (unused for TV_HALF)
    };
    static constexpr int kInput = -2, kBoot = -1, kLinear = -3, kTable = -4;
    static constexpr size_t kMaxTables = 65535;
    void check_open() const;
    void check_id(uint32_t id) const;
    uint32_t push(Kind k, int gate, uint32_t a, uint32_t b, uint32_t c, Ref r);
    Ref new_phys(int gate, Ref x, Ref y);
    uint32_t table_id(int cls, TvKind kind, uint32_t lut);

    std::vector<Node> nodes_;
    std::vector<Ref> ref_;       // per node id: what it resolves to
    std::vector<Phys> phys_;
    std::vector<uint32_t> outs_;
    std::vector<Lin> lin_;
    std::vector<int8_t> fclass_;                                    // per node id: func_class
    std::vector<std::vector<uint64_t>> luts_;                       // distinct LUTs
    std::map<std::vector<uint64_t>, uint32_t> lut_ids_;
    std::vector<TableSpec> tabs_[3];                                // per launch class (0 unused): distinct tables
    std::map<std::pair<int, uint32_t>, uint32_t> tab_ids_[3];       // (kind, lut) -> index in tabs_[cls]
    std::map<std::pair<uint32_t, int>, uint32_t> stage1_;           // (operand phys, class) -> shared first stage
    size_t n_in_ = 0, max_slots_ = 0;
    uint32_t max_ptmod_ = 0;  // the largest plaintext modulus of a multi-input gate
    bool finalized_ = false;
    uint64_t serial_ = 0;
    // after finalize(): phys indices of the bootstrapped rows and of the LINEAR rows in pool-row order, first row
    // per level (+ end), and per level: class widths, first-stage count of class 2, first slot, first LINEAR
    struct LevelPlan {
        size_t w[4], arb1, slot, lin, xw;
        std::vector<std::pair<uint32_t, size_t>> extra;  // (ptmod, width) of the gate classes after class 2; xw their sum
    };
    std::vector<uint32_t> slots_, lins_;
    std::vector<size_t> level_row_;
    std::vector<LevelPlan> plan_;
};

}  // namespace fhe_amd
