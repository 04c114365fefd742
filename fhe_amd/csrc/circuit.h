// circuit.h -- boolean circuits over the gate bootstrap: the DAG a caller builds, its level plan (host
// only, no device or context), and the per-node descriptor the indexed prep kernels read.
//
// The counterpart of the reference's BatchDAG (src/binfhe/include/batch/binfhe-batch.h:229-279), whose
// Execute runs one gate at a time (src/binfhe/lib/batch/batch.cpp:429-482).  Here every level of the DAG
// is one prep + blind rotation + key switch over all of its gates, whatever their types (DESIGN.md §4 "Circuits").
//
// Not supported, refused when the node is added (std::invalid_argument, FHE_HIP_ERR_INVALID_PARAM):
//   - the multi-input gates AND3 / OR3 / AND4 / OR4 / MAJORITY (their own lv / uv / b_const: no shared launch),
//   - EvalFunc nodes,
//   - inputs mod Q (every input is a ciphertext mod q of dimension n).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "params.h"

namespace fhe_amd {

// The ciphertext one slot of a level launch bootstraps (bootstrap.hip PoolFetch):
//   ct = sum_j (-1)^{neg_j} pool[src_j B + inst] + (0, boff_pre) mod q, doubled when dbl, then b += bshift.
// boff_pre: q/4 per negated operand (EvalNOT, binfhe-base-scheme.cpp:223-236) plus q/4 for BOOTSTRAP (:201);
// bshift = q1(AND) - q1(gate) mod q moves the gate's window onto the level's one launch window (AND's).
struct CircuitSlot {
    uint32_t src0, src1;  // pool rows of the operands (src1 unused when kOne)
    uint32_t flags;
    uint32_t boff_pre, bshift;
    static constexpr uint32_t kNeg0 = 1, kNeg1 = 2, kDbl = 4, kOne = 8;
};

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
    uint32_t add_cmux(uint32_t c0, uint32_t c1, uint32_t sel);   // sel ? c1 : c0, as Engine::cmux_levels folds it
    uint32_t add_bootstrap(uint32_t x);                          // BinFHEScheme::Bootstrap
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
    size_t num_rows() const { return n_in_ + slots_.size(); }
    void node_row(uint32_t id, uint32_t* row, uint32_t* neg) const;
    // Descriptors in pool-row order (slot i writes row num_inputs() + i) for a parameter set: gate codes,
    // negations and the fold constants of gate_fold(p, gate, AND)
    std::vector<CircuitSlot> slots(const Params& p) const;
    std::vector<CircuitOut> outputs() const;

private:
    enum Kind : uint8_t { K_INPUT, K_NOT, K_GATE, K_CMUX, K_BOOTSTRAP };
    struct Node {
        Kind kind;
        int gate;
        uint32_t in[3];
    };
    struct Ref {  // a bootstrapped node or input, possibly negated
        uint32_t phys, neg;
    };
    struct Phys {  // an input (gate = kInput) or one bootstrap: a 2-input gate, or BOOTSTRAP (gate = kBoot)
        int gate;
        Ref x, y;
        uint32_t level, row;
    };
    static constexpr int kInput = -2, kBoot = -1;
    void check_open() const;
    void check_id(uint32_t id) const;
    uint32_t push(Kind k, int gate, uint32_t a, uint32_t b, uint32_t c, Ref r);
    Ref new_phys(int gate, Ref x, Ref y);

    std::vector<Node> nodes_;
    std::vector<Ref> ref_;       // per node id: what it resolves to
    std::vector<Phys> phys_;
    std::vector<uint32_t> outs_;
    size_t n_in_ = 0, max_slots_ = 0;
    bool finalized_ = false;
    uint64_t serial_ = 0;
    // after finalize(): phys indices in pool-row order past the inputs, first row per level (+ end)
    std::vector<uint32_t> slots_;
    std::vector<size_t> level_row_;
};

}  // namespace fhe_amd
