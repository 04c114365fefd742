// circuit.cpp -- circuit DAG and level plan (circuit.h).  Host only.
#include "circuit.h"

#include <algorithm>
#include <atomic>
#include <stdexcept>

namespace fhe_amd {

namespace {
constexpr uint64_t kBeta = 128;  // BinFHEContext::GetBeta (binfhecontext.h:445-447)

bool two_input(int gate) {
    switch (gate) {
        case G_OR: case G_AND: case G_NOR: case G_NAND: case G_XOR: case G_XNOR: case G_XOR_FAST: case G_XNOR_FAST:
            return true;
        default:
            return false;
    }
}

bool multi_input(int gate) {
    return gate == G_MAJORITY || gate == G_AND3 || gate == G_OR3 || gate == G_AND4 || gate == G_OR4;
}
}  // namespace

// checkInputFunction (binfhe-base-scheme.h:245-260): 0 negacyclic, 1 periodic, 2 arbitrary
int lut_property(const uint64_t* lut, uint64_t len, uint64_t mod) {
    const uint64_t mid = len / 2;
    if (lut[0] == mod - lut[mid]) {
        for (uint64_t i = 1; i < mid; ++i)
            if (lut[i] != mod - lut[mid + i]) return 2;
        return 0;
    }
    if (lut[0] == lut[mid]) {
        for (uint64_t i = 1; i < mid; ++i)
            if (lut[i] != lut[mid + i]) return 2;
        return 1;
    }
    return 2;
}

std::vector<uint64_t> tv_values(TvKind kind, const uint64_t* lut, uint64_t lutlen, uint64_t q, uint64_t fmod) {
    std::vector<uint64_t> f(q);
    for (uint64_t x = 0; x < q; ++x) {
        switch (kind) {
            case TV_LUT: f[x] = lut[x]; break;                                                       // :254-256
            case TV_LUT_ANTI:                                                                        // :302-307, 324-329
                f[x] = x < (q >> 1) ? lut[x % lutlen] : fmod - lut[(x - q / 2) % lutlen];
                break;
            case TV_HALF: f[x] = x < (q >> 1) ? fmod - (q >> 2) : (q >> 2); break;                  // f0/f1 :285-290
            case TV_FLOOR2:                                                                          // f2 :361-368
                f[x] = x < (q >> 2) ? fmod - (q >> 1) - x : (x < 3 * (q >> 2) ? x : fmod + (q >> 1) - x);
                break;
            case TV_SIGN: f[x] = x < q / 2 ? fmod / 4 : fmod - fmod / 4; break;                      // f3 :413-416
            case TV_SIGN_SS: f[x] = x < q / 2 ? fmod - fmod / 4 : fmod / 4; break;                   // :421-424
        }
    }
    return f;
}

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

GateWindow gate_window(const Params& p, int gate, uint32_t ptmod) {
    if (!two_input(gate) && !multi_input(gate)) throw std::invalid_argument("gate window: unsupported gate");
    if (ptmod < 2 || 2ull * ptmod > p.q) throw std::invalid_argument("plaintext modulus out of range");
    const uint64_t q = p.q, q1 = p.gate_const(gate), value = p.Q / (2ull * ptmod) + 1;
    return GateWindow{q1, value, multi_input(gate) ? value : (p.Q >> 3) + 1, (p.gate_const(G_AND) + q - q1) % q};
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
    fclass_.push_back(-1);
    return (uint32_t)(nodes_.size() - 1);
}

Circuit::Ref Circuit::new_phys(int gate, Ref x, Ref y) {
    if (two_input(gate) && x.phys == y.phys && x.neg == y.neg)
        throw std::invalid_argument("circuit: a gate's input ciphertexts must be independent");
    phys_.push_back(Phys{gate, x, y, 0, 0, 0, 0, 0, {Ref{0, 0}, Ref{0, 0}}, 0, 0});
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

uint32_t Circuit::add_gate_multi(int gate, const uint32_t* xs, size_t k, uint32_t ptmod) {
    check_open();
    if (!multi_input(gate))
        throw std::invalid_argument("circuit: a multi-input node is AND3, OR3, AND4, OR4 or MAJORITY");
    if (k < 2 || k > 4) throw std::invalid_argument("EvalBinGate(ctvector): 2 to 4 ciphertexts");
    if (!xs) throw std::invalid_argument("circuit: a multi-input node needs operands");
    if (ptmod < 2) throw std::invalid_argument("plaintext modulus out of range");
    Ref r[4] = {};
    for (size_t j = 0; j < k; ++j) {
        check_id(xs[j]);
        r[j] = ref_[xs[j]];
        for (size_t i = 0; i < j; ++i)  // the reference's pairwise check (binfhe-base-scheme.cpp:136-143)
            if (r[i].phys == r[j].phys && r[i].neg == r[j].neg)
                throw std::invalid_argument("circuit: a gate's input ciphertexts must be independent");
    }
    if (nodes_.size() >= 0x7fffffffu) throw std::invalid_argument("circuit too large");
    // every refusal is above: from here on the node is added
    const Ref out = new_phys(gate, r[0], r[1]);
    Phys& p = phys_[out.phys];
    p.z[0] = r[2];
    p.z[1] = r[3];
    p.k = (uint32_t)k;
    p.ptmod = ptmod;
    max_ptmod_ = std::max(max_ptmod_, ptmod);
    return push(K_MULTI, gate, xs[0], xs[1], k > 2 ? xs[2] : 0, out);
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

uint32_t Circuit::table_id(int cls, TvKind kind, uint32_t lut) {
    const auto key = std::make_pair((int)kind, lut);
    const auto it = tab_ids_[cls].find(key);
    if (it != tab_ids_[cls].end()) return it->second;
    const uint32_t id = (uint32_t)tabs_[cls].size();
    tabs_[cls].push_back(TableSpec{kind, lut});
    tab_ids_[cls][key] = id;
    return id;
}

uint32_t Circuit::add_func(uint32_t x, const uint64_t* lut, size_t len) {
    check_open();
    check_id(x);
    if (!lut) throw std::invalid_argument("circuit: FUNC needs a LUT");
    if (len < 4 || (len & (len - 1)) || len > (1u << 16))
        throw std::invalid_argument("circuit: a FUNC node's LUT length must be a power of two >= 4");
    for (size_t i = 0; i < len; ++i)
        if (lut[i] >= len) throw std::invalid_argument("circuit: a FUNC node's LUT values must be below its length");
    const Ref op = ref_[x];
    if (op.neg)
        throw std::invalid_argument("circuit: FUNC of a NOT alias is not supported (a negation mod q does not survive the lift to 2q)");
    if (nodes_.size() >= 0x7fffffffu) throw std::invalid_argument("circuit too large");
    const int prop = lut_property(lut, len, len);
    const int cls = prop == 2 ? 2 : 1;
    if (tabs_[cls].size() + 2 > kMaxTables) throw std::invalid_argument("circuit: more than 65535 tables in one launch class");
    // every refusal is above: from here on the node is added
    std::vector<uint64_t> v(lut, lut + len);
    uint32_t lid;
    const auto it = lut_ids_.find(v);
    if (it != lut_ids_.end()) {
        lid = it->second;
    } else {
        lid = (uint32_t)luts_.size();
        lut_ids_[v] = lid;
        luts_.push_back(std::move(v));
    }
    Ref out;
    if (prop == 0) {  // negacyclic: one bootstrap of x + beta with the LUT as table (:253-259)
        out = new_phys(kTable, op, op);
        Phys& p = phys_[out.phys];
        p.cls = 1;
        p.stage = 2;
        p.aux = table_id(1, TV_LUT, lid);
    } else {  // periodic (:309-331) at q, arbitrary (:261-307) at 2q: the first stage is shared per operand and class
        const auto key = std::make_pair(op.phys, cls);
        const auto s1 = stage1_.find(key);
        Ref first;
        if (s1 != stage1_.end()) {
            first = Ref{s1->second, 0};
        } else {
            first = new_phys(kTable, op, op);
            Phys& p = phys_[first.phys];
            p.cls = (uint8_t)cls;
            p.stage = 1;
            p.aux = table_id(cls, TV_HALF, 0);
            stage1_[key] = first.phys;
        }
        out = new_phys(kTable, op, first);
        Phys& p = phys_[out.phys];
        p.cls = (uint8_t)cls;
        p.stage = 2;
        p.aux = table_id(cls, TV_LUT_ANTI, lid);
    }
    const uint32_t id = push(K_FUNC, 0, x, 0, 0, out);
    fclass_[id] = (int8_t)prop;
    return id;
}

uint32_t Circuit::add_linear(const uint32_t* xs, const int* signs, size_t k, uint64_t c) {
    check_open();
    if (k < 1 || k > 4) throw std::invalid_argument("circuit: LINEAR takes 1 to 4 operands");
    if (!xs) throw std::invalid_argument("circuit: LINEAR needs operands");
    Lin ln{};
    ln.k = (uint32_t)k;
    ln.c = c;
    for (size_t j = 0; j < k; ++j) {
        check_id(xs[j]);
        Ref r = ref_[xs[j]];
        if (phys_[r.phys].gate == kLinear)
            throw std::invalid_argument("circuit: a LINEAR operand of LINEAR is not supported (flatten the sum)");
        // the sign in bit 1, next to the operand's own negation in bit 0 (linears() folds both)
        r.neg |= (signs && signs[j] < 0) ? 2u : 0u;
        ln.x[j] = r;
    }
    if (nodes_.size() >= 0x7fffffffu) throw std::invalid_argument("circuit too large");
    const Ref out = new_phys(kLinear, Ref{ln.x[0].phys, 0}, Ref{0, 0});
    phys_[out.phys].aux = (uint32_t)lin_.size();
    lin_.push_back(ln);
    return push(K_LINEAR, 0, xs[0], 0, 0, out);
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
    uint32_t top = 0;
    for (Phys& p : phys_) {
        if (p.gate == kInput) {
            p.level = 0;
        } else if (p.gate == kLinear) {  // no bootstrap: the highest level of its operands
            const Lin& ln = lin_[p.aux];
            p.level = 0;
            for (uint32_t j = 0; j < ln.k; ++j) p.level = std::max(p.level, phys_[ln.x[j].phys].level);
        } else {
            p.level = p.gate == kBoot ? phys_[p.x.phys].level : std::max(phys_[p.x.phys].level, phys_[p.y.phys].level);
            for (uint32_t j = 2; j < p.k; ++j) p.level = std::max(p.level, phys_[p.z[j - 2].phys].level);
            ++p.level;
        }
        top = std::max(top, p.level);
    }
    // a level's rows: class 0 (with the multi-input gates at plaintext modulus 4), class 1, class 2 (first stages,
    // then second stages), the gate classes of the other plaintext moduli in ascending order, LINEAR; level 0: the
    // inputs first.  Groups 0..3 and 5 are fixed; group 4 is split by modulus.
    auto order = [](const Phys& p) -> int {
        if (p.gate == kLinear) return 5;
        if (p.ptmod && p.ptmod != 4) return 4;
        if (p.gate == kInput || p.cls == 0) return 0;
        return p.cls == 1 ? 1 : 1 + p.stage;
    };
    std::vector<size_t> cnt((size_t)(top + 1) * 6, 0);
    std::vector<std::map<uint32_t, size_t>> extra(top + 1);  // per level: ptmod -> width, then -> next row
    for (const Phys& p : phys_) {
        const int o = order(p);
        ++cnt[(size_t)p.level * 6 + o];
        if (o == 4) ++extra[p.level][p.ptmod];
    }
    level_row_.assign(top + 2, 0);
    plan_.assign(top + 1, LevelPlan{});
    std::vector<size_t> next((size_t)(top + 1) * 6, 0);
    size_t n_slots = 0, n_lins = 0;
    for (uint32_t l = 0; l <= top; ++l) {
        const size_t* c = &cnt[(size_t)l * 6];
        LevelPlan& lp = plan_[l];
        size_t row = level_row_[l];
        for (int o = 0; o < 6; ++o) {
            next[(size_t)l * 6 + o] = row;
            if (o == 4) {
                for (auto& e : extra[l]) {
                    lp.extra.emplace_back(e.first, e.second);
                    const size_t width = e.second;
                    e.second = row;
                    row += width;
                }
            } else {
                row += c[o];
            }
        }
        level_row_[l + 1] = row;
        lp.w[0] = l ? c[0] : 0;
        lp.w[1] = c[1];
        lp.w[2] = c[2] + c[3];
        lp.w[3] = c[5];
        lp.arb1 = c[2];
        lp.slot = n_slots;
        lp.lin = n_lins;
        lp.xw = c[4];
        n_slots += lp.w[0] + lp.w[1] + lp.w[2] + lp.xw;
        n_lins += lp.w[3];
    }
    slots_.assign(n_slots, 0);
    lins_.assign(n_lins, 0);
    for (uint32_t i = 0; i < phys_.size(); ++i) {
        Phys& p = phys_[i];
        const int o = order(p);
        p.row = (uint32_t)(o == 4 ? extra[p.level][p.ptmod]++ : next[(size_t)p.level * 6 + o]++);
        if (p.gate == kInput) continue;
        // bootstrapped rows come first in a level (after the inputs in level 0), LINEAR rows last
        const LevelPlan& lp = plan_[p.level];
        const size_t in_level = p.row - level_row_[p.level] - (p.level ? 0 : n_in_);
        if (p.gate == kLinear) lins_[lp.lin + in_level - (lp.w[0] + lp.w[1] + lp.w[2] + lp.xw)] = i;
        else slots_[lp.slot + in_level] = i;
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

void Circuit::level_classes(size_t level, size_t w[4]) const {
    if (!finalized_) throw std::logic_error("circuit is not finalized");
    if (level >= plan_.size()) throw std::invalid_argument("circuit: no such level");
    for (int j = 0; j < 4; ++j) w[j] = plan_[level].w[j];
}

const std::vector<std::pair<uint32_t, size_t>>& Circuit::level_gate_classes(size_t level) const {
    if (!finalized_) throw std::logic_error("circuit is not finalized");
    if (level >= plan_.size()) throw std::invalid_argument("circuit: no such level");
    return plan_[level].extra;
}

size_t Circuit::level_arb_stage1(size_t level) const {
    if (!finalized_) throw std::logic_error("circuit is not finalized");
    if (level >= plan_.size()) throw std::invalid_argument("circuit: no such level");
    return plan_[level].arb1;
}

size_t Circuit::level_slot(size_t level) const {
    if (!finalized_) throw std::logic_error("circuit is not finalized");
    if (level >= plan_.size()) throw std::invalid_argument("circuit: no such level");
    return plan_[level].slot;
}

size_t Circuit::level_linear(size_t level) const {
    if (!finalized_) throw std::logic_error("circuit is not finalized");
    if (level >= plan_.size()) throw std::invalid_argument("circuit: no such level");
    return plan_[level].lin;
}

void Circuit::node_row(uint32_t id, uint32_t* row, uint32_t* neg) const {
    if (!finalized_) throw std::logic_error("circuit is not finalized");
    check_id(id);
    *row = phys_[ref_[id].phys].row;
    *neg = ref_[id].neg;
}

int Circuit::func_class(uint32_t id) const {
    check_id(id);
    return fclass_[id];
}

std::vector<CircuitSlot> Circuit::slots(const Params& p) const {
    if (!finalized_) throw std::logic_error("circuit is not finalized");
    std::vector<CircuitSlot> out(slots_.size());
    const uint32_t q = p.q, q4 = q >> 2;
    for (size_t i = 0; i < slots_.size(); ++i) {
        const Phys& ph = phys_[slots_[i]];
        CircuitSlot& d = out[i];
        d = CircuitSlot{};
        d.src[0] = phys_[ph.x.phys].row;
        d.k = 1;
        if (ph.gate == kTable) {  // EvalFunc's stages (fb.cpp eval_func_device), at the class's modulus
            const uint32_t cm = table_ctmod(p, ph.cls), beta = (uint32_t)(kBeta % cm);
            d.flags = ph.aux << CircuitSlot::kTableShift;
            if (ph.y.phys == ph.x.phys) {  // x + beta: negacyclic, or a first stage
                d.boff_pre = beta;
            } else {  // x - first stage + beta - q/4 (periodic) or - q/2 (arbitrary, mod 2q)
                d.src[1] = phys_[ph.y.phys].row;
                d.k = 2;
                d.flags |= CircuitSlot::kNeg << 1;
                d.boff_pre = (beta + cm - (ph.cls == 2 ? q >> 1 : q4)) % cm;
            }
            continue;
        }
        if (ph.gate == kBoot) {  // Bootstrap: ct + q/4 in the AND window (binfhe-base-scheme.cpp:190-205)
            d.flags = ph.x.neg ? CircuitSlot::kNeg : 0u;
            d.boff_pre = ((ph.x.neg ? q4 : 0u) + q4) % q;
            continue;
        }
        // a gate over k operands: EvalNOT of an operand is a sign flip and q/4 (:223-236)
        const Ref ops[4] = {ph.x, ph.y, ph.z[0], ph.z[1]};
        d.k = ph.ptmod ? ph.k : 2;
        for (uint32_t j = 0; j < d.k; ++j) {
            d.src[j] = phys_[ops[j].phys].row;
            if (ops[j].neg) {
                d.flags |= CircuitSlot::kNeg << j;
                d.boff_pre = (d.boff_pre + q4) % q;
            }
        }
        if (ph.ptmod) {  // multi-input: the sum as it is, its window moved onto AND's
            d.bshift = (uint32_t)((p.gate_const(G_AND) + q - p.gate_const(ph.gate)) % q);
            continue;
        }
        const GateFold f = gate_fold(p, ph.gate, G_AND);
        if (f.dbl) d.flags |= CircuitSlot::kDbl;
        d.bshift = f.bshift;
    }
    for (CircuitSlot& d : out) {  // the rows PoolFetch fetches in pairs
        if (d.k == 1) d.src[1] = d.src[0];
        if (d.k == 3) d.src[3] = d.src[2];
    }
    return out;
}

std::vector<CircuitLinear> Circuit::linears(const Params& p) const {
    if (!finalized_) throw std::logic_error("circuit is not finalized");
    std::vector<CircuitLinear> out(lins_.size());
    const uint64_t q = p.q, q4 = q >> 2;
    for (size_t i = 0; i < lins_.size(); ++i) {
        const Lin& ln = lin_[phys_[lins_[i]].aux];
        CircuitLinear& d = out[i];
        d = CircuitLinear{};
        d.k = ln.k;
        uint64_t c = ln.c % q;
        for (uint32_t j = 0; j < ln.k; ++j) {
            const uint32_t alias = ln.x[j].neg & 1u, minus = (ln.x[j].neg >> 1) & 1u;
            d.src[j] = phys_[ln.x[j].phys].row;
            // +NOT(x) = -x + q/4, -NOT(x) = x - q/4 (EvalNOT, binfhe-base-scheme.cpp:223-236)
            if (alias) c = (c + (minus ? q - q4 : q4)) % q;
            if (alias ^ minus) d.neg_mask |= 1u << j;
        }
        d.c = (uint32_t)c;
    }
    return out;
}

std::vector<CircuitOut> Circuit::outputs() const {
    if (!finalized_) throw std::logic_error("circuit is not finalized");
    std::vector<CircuitOut> out(outs_.size());
    for (size_t i = 0; i < outs_.size(); ++i) out[i] = CircuitOut{phys_[ref_[outs_[i]].phys].row, ref_[outs_[i]].neg};
    return out;
}

size_t Circuit::num_tables(int cls) const {
    if (cls != 1 && cls != 2) throw std::invalid_argument("circuit: table classes are 1 and 2");
    return tabs_[cls].size();
}

void Circuit::check_params(const Params& p) const {
    if (2ull * max_ptmod_ > p.q)  // Engine::gate_args' rule for the per-gate path
        throw std::invalid_argument("plaintext modulus out of range");
    for (const auto& l : luts_)
        if (l.size() != p.q) throw std::invalid_argument("circuit: a FUNC node's LUT length must equal the ciphertext modulus q");
    if (!tabs_[2].empty()) {
        if (p.q > p.N)
            throw std::invalid_argument("ERROR: ciphertext modulus q needs to be <= ring dimension for arbitrary function evaluation");
        if (p.method == M_AP)  // EvalAcc DM reads a_i modulo the parameter q (rgsw-acc-dm.cpp:64-69)
            throw std::invalid_argument("AP accumulator: ciphertext modulus must be q");
    }
}

std::vector<uint64_t> Circuit::tables(const Params& p, int cls) const {
    const size_t nt = num_tables(cls);
    check_params(p);
    const uint64_t cm = table_ctmod(p, cls), scale = p.Q / cm;  // fmod = ctmod in every stage of EvalFunc
    std::vector<uint64_t> out(nt * cm);
    for (size_t t = 0; t < nt; ++t) {
        const TableSpec& ts = tabs_[cls][t];
        const bool lut = ts.kind != TV_HALF;
        const std::vector<uint64_t> f = tv_values(ts.kind, lut ? luts_[ts.lut].data() : nullptr, lut ? luts_[ts.lut].size() : 0, cm, cm);
        for (uint64_t x = 0; x < cm; ++x) out[t * cm + x] = scale * f[x];
    }
    return out;
}

}  // namespace fhe_amd
