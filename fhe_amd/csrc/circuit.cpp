// circuit.cpp -- circuit DAG and level plan (circuit.h).  Host only.
#include "circuit.h"

#include <algorithm>
#include <atomic>
#include <stdexcept>

namespace fhe_amd {

namespace {
bool two_input(int gate) {
    switch (gate) {
        case G_OR: case G_AND: case G_NOR: case G_NAND: case G_XOR: case G_XNOR: case G_XOR_FAST: case G_XNOR_FAST:
            return true;
        default:
            return false;
    }
}
}  // namespace

GateFold gate_fold(const Params& p, int gate, int ref_gate) {
    if (!two_input(gate) || !two_input(ref_gate))
        throw std::invalid_argument("gate fold: 2-input gates only (OR, AND, NOR, NAND, XOR, XNOR)");
    const uint64_t q = p.q, q1 = p.gate_const(gate), qr = p.gate_const(ref_gate);
    GateFold f;
    f.dbl = (gate == G_XOR || gate == G_XNOR || gate == G_XOR_FAST || gate == G_XNOR_FAST) ? 1 : 0;
    f.q1 = (uint32_t)q1;
    f.bshift = (uint32_t)((qr + q - q1) % q);
    return f;
}

void Circuit::check_open() const {
    if (finalized_) throw std::invalid_argument("circuit is finalized: no node or output can be added");
}

void Circuit::check_id(uint32_t id) const {
    if (id >= nodes_.size()) throw std::invalid_argument("circuit: unknown node id");
}

uint32_t Circuit::push(Kind k, int gate, uint32_t a, uint32_t b, uint32_t c, Ref r) {
    if (nodes_.size() >= 0x7fffffffu) throw std::invalid_argument("circuit too large");
    nodes_.push_back(Node{k, gate, {a, b, c}});
    ref_.push_back(r);
    return (uint32_t)(nodes_.size() - 1);
}

Circuit::Ref Circuit::new_phys(int gate, Ref x, Ref y) {
    if (gate != kInput && gate != kBoot && x.phys == y.phys && x.neg == y.neg)
        throw std::invalid_argument("circuit: a gate's input ciphertexts must be independent");
    phys_.push_back(Phys{gate, x, y, 0, 0});
    return Ref{(uint32_t)(phys_.size() - 1), 0};
}

uint32_t Circuit::add_input() {
    check_open();
    const Ref r = new_phys(kInput, Ref{0, 0}, Ref{0, 0});
    ++n_in_;
    return push(K_INPUT, 0, 0, 0, 0, r);
}

uint32_t Circuit::add_not(uint32_t x) {
    check_open();
    check_id(x);
    return push(K_NOT, 0, x, 0, 0, Ref{ref_[x].phys, ref_[x].neg ^ 1u});
}

uint32_t Circuit::add_gate(int gate, uint32_t x, uint32_t y) {
    check_open();
    if (!two_input(gate))
        throw std::invalid_argument("circuit: 2-input gates only (AND3, OR3, AND4, OR4, MAJORITY are not supported)");
    check_id(x);
    check_id(y);
    return push(K_GATE, gate, x, y, 0, new_phys(gate, ref_[x], ref_[y]));
}

uint32_t Circuit::add_cmux(uint32_t c0, uint32_t c1, uint32_t sel) {
    check_open();
    check_id(c0);
    check_id(c1);
    check_id(sel);
    // NAND(NAND(c0, NOT sel), NAND(c1, sel)) (binfhe-base-scheme.cpp:176-182); nothing is added if either
    // first-level NAND is refused
    const Ref s = ref_[sel], ns{s.phys, s.neg ^ 1u};
    const size_t mark = phys_.size();
    try {
        const Ref lo = new_phys(G_NAND, ref_[c0], ns);
        const Ref hi = new_phys(G_NAND, ref_[c1], s);
        return push(K_CMUX, G_CMUX, c0, c1, sel, new_phys(G_NAND, lo, hi));
    } catch (...) {
        phys_.resize(mark);
        throw;
    }
}

uint32_t Circuit::add_bootstrap(uint32_t x) {
    check_open();
    check_id(x);
    return push(K_BOOTSTRAP, 0, x, 0, 0, new_phys(kBoot, ref_[x], Ref{0, 0}));
}

void Circuit::mark_output(uint32_t id) {
    check_open();
    check_id(id);
    outs_.push_back(id);
}

void Circuit::finalize() {
    check_open();
    for (const Node& nd : nodes_)  // ids were checked as they were added; a finalized plan never indexes past them
        for (uint32_t j = 0; j < 3; ++j) check_id(nd.in[j]);
    // operands precede their users in phys_, so one pass levelises
    uint32_t top = 0, in_row = 0;
    for (Phys& p : phys_) {
        if (p.gate == kInput) {
            p.level = 0;
            p.row = in_row++;
            continue;
        }
        p.level = 1 + (p.gate == kBoot ? phys_[p.x.phys].level : std::max(phys_[p.x.phys].level, phys_[p.y.phys].level));
        top = std::max(top, p.level);
    }
    std::vector<size_t> width(top + 1, 0);
    width[0] = n_in_;
    for (const Phys& p : phys_)
        if (p.gate != kInput) ++width[p.level];
    level_row_.assign(top + 2, 0);
    for (uint32_t l = 0; l <= top; ++l) level_row_[l + 1] = level_row_[l] + width[l];
    std::vector<size_t> next(level_row_.begin(), level_row_.end() - 1);
    slots_.assign(phys_.size() - n_in_, 0);
    for (uint32_t i = 0; i < phys_.size(); ++i) {
        Phys& p = phys_[i];
        if (p.gate == kInput) continue;
        p.row = (uint32_t)next[p.level]++;
        slots_[p.row - n_in_] = i;
    }
    static std::atomic<uint64_t> counter{0};
    serial_ = ++counter;
    finalized_ = true;
}

size_t Circuit::level_width(size_t level) const {
    if (!finalized_) throw std::logic_error("circuit is not finalized");
    if (level + 1 >= level_row_.size()) throw std::invalid_argument("circuit: no such level");
    return level_row_[level + 1] - level_row_[level];
}

size_t Circuit::level_row(size_t level) const {
    if (!finalized_) throw std::logic_error("circuit is not finalized");
    if (level + 1 >= level_row_.size()) throw std::invalid_argument("circuit: no such level");
    return level_row_[level];
}

void Circuit::node_row(uint32_t id, uint32_t* row, uint32_t* neg) const {
    if (!finalized_) throw std::logic_error("circuit is not finalized");
    check_id(id);
    *row = phys_[ref_[id].phys].row;
    *neg = ref_[id].neg;
}

std::vector<CircuitSlot> Circuit::slots(const Params& p) const {
    if (!finalized_) throw std::logic_error("circuit is not finalized");
    std::vector<CircuitSlot> out(slots_.size());
    const uint32_t q = p.q, q4 = q >> 2;
    for (size_t i = 0; i < slots_.size(); ++i) {
        const Phys& ph = phys_[slots_[i]];
        CircuitSlot& d = out[i];
        d.src0 = phys_[ph.x.phys].row;
        d.flags = ph.x.neg ? CircuitSlot::kNeg0 : 0u;
        d.boff_pre = ph.x.neg ? q4 : 0u;
        if (ph.gate == kBoot) {  // Bootstrap: ct + q/4 in the AND window (binfhe-base-scheme.cpp:190-205)
            d.src1 = d.src0;
            d.flags |= CircuitSlot::kOne;
            d.boff_pre = (d.boff_pre + q4) % q;
            d.bshift = 0;
            continue;
        }
        d.src1 = phys_[ph.y.phys].row;
        if (ph.y.neg) {
            d.flags |= CircuitSlot::kNeg1;
            d.boff_pre = (d.boff_pre + q4) % q;
        }
        const GateFold f = gate_fold(p, ph.gate, G_AND);
        if (f.dbl) d.flags |= CircuitSlot::kDbl;
        d.bshift = f.bshift;
    }
    return out;
}

std::vector<CircuitOut> Circuit::outputs() const {
    if (!finalized_) throw std::logic_error("circuit is not finalized");
    std::vector<CircuitOut> out(outs_.size());
    for (size_t i = 0; i < outs_.size(); ++i) out[i] = CircuitOut{phys_[ref_[outs_[i]].phys].row, ref_[outs_[i]].neg};
    return out;
}

}  // namespace fhe_amd
