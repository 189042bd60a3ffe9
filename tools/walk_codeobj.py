"""
What the walk machine (umpa_amd/csrc/umpa_walk.h) compiled to, per kernel that inlines it (no GPU needed).

    python tools/walk_codeobj.py LIB [LIB ...]        # libumpa_hip.so builds, or already unbundled code objects

Per library and kernel: VGPRs, scratch bytes, spilled VGPRs, the kernel's static count of vector-ALU instructions and of
register copies among them (v_mov_b32 / v_mov_b64 / v_accvgpr moves), and the same two counts inside the walk loop -- the
innermost loop of the kernel that holds every store to the LDS memo (walk_feed is the only code that writes it), that is
`while (w.phase < PH_FIT)` with the cost evaluation and the inlined walk_feed copies.
"""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_coverage import _run, llvm_tool   # noqa: E402
from codeobj_diff import code_object, kernels   # noqa: E402

KERNELS = ("replay_walk_kernel<1, 10, false>", "replay_walk_kernel<1, 20, false>", "replay_walk_kernel<0, 0, false>",
           "replay_walk_kernel<1, 12, true>", "replay_walk_kernel<1, 24, true>", "replay_cost_kernel<1>",
           "match_direct_kernel<1, false, 5>", "match_staged_kernel<1, false, 5>")

_VALU = re.compile(r"^v_")
_NOT_ALU = ("v_nop", "v_readlane", "v_readfirstlane", "v_writelane")
_MOVES = ("v_mov_b32", "v_mov_b64", "v_accvgpr_mov", "v_accvgpr_read", "v_accvgpr_write")


def disassemble(co, symbol):
    """[(address, mnemonic, operands)] of one function"""
    text = _run([llvm_tool("llvm-objdump"), "-d", "--no-show-raw-insn", "--disassemble-symbols=" + symbol, co])
    out = []
    for line in text.splitlines():
        m = re.match(r"\s+(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):", line)
        if m:
            out.append((int(m.group(3), 16), m.group(1), m.group(2)))
    return out


def count(ins):
    valu = [i for i in ins if _VALU.match(i[1]) and not i[1].startswith(_NOT_ALU)]
    return len(valu), sum(1 for i in valu if i[1].startswith(_MOVES))


def walk_loop(ins):
    """the instructions of the innermost loop that holds every ds_write_b64 of the function (None: no such loop)"""
    stores = [a for a, m, _ in ins if m.startswith("ds_write_b64") or m.startswith("ds_store_b64")]
    if not stores:
        return None
    best = None
    for k, (a, m, ops) in enumerate(ins):
        if m.startswith(("s_cbranch", "s_branch")):
            # the branch offset is in dwords from the next instruction; objdump prints it as a signed or a 16-bit number
            t = re.match(r"(-?\d+)", ops)
            if not t:
                continue
            off = int(t.group(1))
            if off >= 32768:
                off -= 65536
            nxt = ins[k + 1][0] if k + 1 < len(ins) else a + 4
            target = nxt + 4 * off
            if target <= a and target <= min(stores) and a >= max(stores):
                if best is None or a - target < best[1] - best[0]:
                    best = (target, a)
    if best is None:
        return None
    return [i for i in ins if best[0] <= i[0] <= best[1]]


def table(lib, td, tag):
    co = code_object(lib, td, tag)
    ks = kernels(co)
    rows = []
    for want in KERNELS:
        for sym, (name, _, res) in ks.items():
            if name.replace("umpa::", "", 1) == want:
                ins = disassemble(co, sym)
                loop = walk_loop(ins)
                rows.append((want, res[0], res[2], res[4]) + count(ins) + (count(loop) if loop else (None, None)))
    return rows


def main(argv):
    if not argv:
        print(__doc__)
        return 2
    with tempfile.TemporaryDirectory() as td:
        for n, lib in enumerate(argv):
            print("# %s" % lib)
            print("%-40s %6s %8s %7s %7s %7s %10s %10s" % ("kernel", "VGPRs", "scratch", "spills", "VALU", "moves", "loop VALU", "loop moves"))
            for r in table(lib, td, "lib%d" % n):
                print("%-40s %6d %8d %7d %7d %7d %10s %10s" % r)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
