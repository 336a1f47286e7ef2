#!/usr/bin/env python3
"""isa_eval_loop.py [--quad] <tag> <poismf_hip.s> [S] : the evaluation loop (one pass over the tile) of every one-wave PG fp32 register kernel
half_sweep_reg_kernel<float, 3, S, 16, 1> in an assembly listing of the PG unit

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -DUSE_FLOAT -DPMF_TU=3 --cuda-device-only -S poismf_amd/csrc/poismf_hip.hip -o poismf_hip.s

One line per S (the format of profiles/r07/isa_eval_loop.txt with two more columns and the per-row gather block): instr = all instructions
of the loop body, VALU = v_* among them; add = unpacked v_add_f32 (DPP adds not counted, they are in "other VALU"); gather-block VALU = the
v_* of the basic block that broadcasts the row's indices and issues its loads (address arithmetic, the swaps of the step pairs and whatever
copies the compiler adds around them).  With S: the loop's VALU instructions of that instance by opcode.  --quad: the same for the quad
engine's kernels half_sweep_quad_kernel<S / 4> (quad_eval.hpp), every S from 4 to 40, so that the two listings line up S by S.

The pass loop is the kernel's inner loop (the blocks LLVM marks "Depth=2"); the script stops if those blocks hold no v_pk_fma_f32, or the
gather block is not found, instead of printing zeros."""
import collections
import re
import sys

STEPS = (12, 16, 20, 24, 28, 32, 36, 40)
LABEL = re.compile(r"^(\.LBB\d+_\d+):")


QUAD_STEPS = tuple(range(4, 41, 4))


def kernels(path, quad=False):
    """{S: lines of the kernel's body}"""
    lines = open(path).read().split("\n")
    out = {}
    for S in QUAD_STEPS if quad else STEPS:
        name = f"_Z22half_sweep_quad_kernelILi{S // 4}EEv8HalfArgsIfE:" if quad else f"_Z21half_sweep_reg_kernelIfLi3ELi{S}ELi16ELi1EEv8HalfArgsIT_E:"
        begin = next(i for i, line in enumerate(lines) if line.startswith(name))
        end = next(i for i in range(begin, len(lines)) if lines[i].startswith(".Lfunc_end"))
        out[S] = lines[begin:end]
    return out


def opcode(line):
    """the instruction's mnemonic, or None for labels, directives, comments and blank lines"""
    line = line.strip()
    if not line or line[0] in ";." or line.endswith(":") or re.match(r"^\.?\w+:", line):
        return None
    return line.split()[0]


def blocks(body):
    """[(label, lines)] : the basic blocks of a kernel, each with its label line first"""
    current = ("entry", [])
    out = [current]
    for line in body:
        m = LABEL.match(line)
        if m:
            current = (m.group(1), [])
            out.append(current)
        current[1].append(line)
    return out


def is_valu(op):
    return op is not None and op.startswith("v_")


def loop_stats(body, S):
    # (a loop header's label line names the parent loop; its own depth is on the comment line below)
    inner = [lines for _, lines in blocks(body) if any("Depth=2" in line for line in lines[:2])]
    ops = [op for lines in inner for op in map(opcode, lines) if op]
    count = collections.Counter(ops)
    assert count["v_pk_fma_f32"] > 0, f"S = {S}: no inner loop with packed multiply-adds found (has the loop nesting changed?)"
    prefixed = lambda prefix: sum(n for op, n in count.items() if op.startswith(prefix) and "dpp" not in op)
    stats = dict(instr=len(ops), valu=sum(1 for op in ops if is_valu(op)), pk_mul=count["v_pk_mul_f32"], pk_fma=count["v_pk_fma_f32"],
                 add=prefixed("v_add_f32"), mov=prefixed("v_mov_b32"), nop=count["s_nop"], cnd=prefixed("v_cndmask"))
    stats["other"] = stats["valu"] - stats["pk_mul"] - stats["pk_fma"] - stats["add"] - stats["mov"] - stats["cnd"]
    return stats, count


def gather_valu(body, S):
    found = [lines for _, lines in blocks(body)
             if any("swizzle(BROADCAST" in line for line in lines) and any("global_load_dwordx4" in line for line in lines)]
    assert found, f"S = {S}: no block that broadcasts indices and loads factor rows"
    return sum(1 for lines in found for op in map(opcode, lines) if is_valu(op))


def main():
    args = [a for a in sys.argv[1:] if a != "--quad"]
    quad = "--quad" in sys.argv[1:]
    tag, path = args[0], args[1]
    detail = int(args[2]) if len(args) > 2 else None
    for S, body in kernels(path, quad).items():
        st, count = loop_stats(body, S)
        print(f"S={S:2d}  {tag} instr {st['instr']:4d}  VALU {st['valu']:4d}  v_pk_mul_f32 {st['pk_mul']:3d}  v_pk_fma_f32 {st['pk_fma']:3d}  "
              f"v_add_f32 {st['add']:3d}  v_mov_b32 {st['mov']:2d}  s_nop {st['nop']:3d}  v_cndmask {st['cnd']:3d}  other VALU {st['other']:3d}  "
              f"gather-block VALU {gather_valu(body, S):3d}")
        if detail == S:
            print({op: n for op, n in count.items() if is_valu(op) and "pk_" not in op})


if __name__ == "__main__":
    main()
