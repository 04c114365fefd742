"""Instruction histograms of the loop blocks of a kernel in a `hipcc -S` (or -save-temps) .s file.

    hipcc -O3 --offload-arch=gfx950 --cuda-device-only -S fhe_amd/csrc/bootstrap.hip -o boot.s
    python tools/loop_hist.py boot.s 'k_blind_rotate_ginxILb0ELb1ELb0E' [top-N opcodes] [min VALU]

Reports every basic block (label to label) of the kernel with at least `min VALU` (default 500) vector ALU
instructions, in program order, with the back-edge that makes it a loop body: the nearest branch at or after
the block's end whose target is the block's own label or an earlier one.  A fully unrolled loop body is one
such block (K1 GINX: the `for i < g.n` body; the LMKCDEY op loop: its EXT and AUTO arms, which share the op
loop's back-edge).  The largest backward span -- what this tool took before -- is the whole function once an
epilogue branches back to a shared exit block.
"""
import collections
import re
import sys

MUL = ('v_mad_i64_i32', 'v_mad_u64_u32', 'v_mul_lo_u32', 'v_mul_hi_u32', 'v_mul_hi_i32', 'v_mul_lo_i32',
       'v_mul_u32_u24', 'v_mul_i32_i24', 'v_mad_u32_u24', 'v_mad_i32_i24')


def kernel_lines(path, kern):
    s = open(path).read()
    m = re.search(r'^(\S*' + re.escape(kern) + r'\S*):', s, re.M)
    if not m:
        raise SystemExit(f"no symbol matching {kern!r} in {path}")
    body = s[m.end():]
    body = body[:body.index('.Lfunc_end')]
    return m.group(1), [l.strip() for l in body.splitlines()]


def blocks(lines):
    """(label, first line, last line) of every basic block: a label starts one, a branch ends one"""
    out, cur, start = [], '<entry>', 0
    for i, l in enumerate(lines):
        m = re.match(r'^(\.LBB\d+_\d+):', l)
        if m:
            out.append((cur, start, i - 1))
            cur, start = m.group(1), i
        elif re.match(r'^s_c?branch', l):
            out.append((cur, start, i))
            cur, start = cur + '+', i + 1
    out.append((cur, start, len(lines) - 1))
    return out


def report(path, kern, top=30, min_valu=500):
    name, lines = kernel_lines(path, kern)
    lab = {m.group(1): i for i, l in enumerate(lines) for m in [re.match(r'^(\.LBB\d+_\d+):', l)] if m}
    print(f"{name}")
    res = []
    for label, a, b in blocks(lines):
        ins = [l for l in lines[a:b + 1] if l and not l.startswith(('.', ';'))]
        c = collections.Counter(l.split()[0] for l in ins)
        valu = sum(v for k, v in c.items() if k.startswith('v_'))
        if valu < min_valu:
            continue
        mul = sum(v for k, v in c.items() if k.startswith(MUL))
        back = None
        for i in range(b, len(lines)):
            m = re.match(r'^s_c?branch\w*\s+(\.LBB\d+_\d+)', lines[i])
            if m and m.group(1) in lab and lab[m.group(1)] <= a:
                back = (i, m.group(1))
                break
        edge = f"back-edge line {back[0]} -> {back[1]}" if back else "no back-edge (straight-line code)"
        print(f"block {label} lines {a}-{b}: {len(ins)} instr, VALU {valu}, multiplies {mul}; {edge}")
        for op, n in c.most_common(top):
            print(f"  {op:30s}{n}")
        res.append((label, valu, mul, c))
    return res


if __name__ == '__main__':
    report(sys.argv[1], sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 30,
           int(sys.argv[4]) if len(sys.argv) > 4 else 500)
