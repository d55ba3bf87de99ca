#!/usr/bin/env python3
"""Compare the gfx950 code objects of two builds of libdronesim.so kernel by kernel: instruction streams
(llvm-objdump -d, addresses and encodings stripped) must be identical for a refactoring that claims "no code change".

    python tools/co_diff.py before.so after.so [--pair OLD=NEW ...] [--fp-only] [--step-bound]

--pair OLD=NEW (repeatable) compares the kernel of before.so whose name contains OLD with the kernel of after.so whose name
contains NEW (each substring must match exactly one kernel), for kernels a refactoring renamed or merged; several OLD may name
the same NEW.  --fp-only compares only the sequence of the floating-point vector instructions' opcodes -- no operands, v_fmac /
v_fma and the _e32 / _e64 encodings spelt alike: "the same arithmetic in the same order" where scalar code, addressing or
register allocation moved.  --step-bound prints the verdict for a change that may touch the step kernel's scalar address arithmetic
and nothing else: every kernel but drone_kernel identical; every drone_kernel instance with its instruction count and its
multiset of opcodes, differing lines only among s_add* / s_lshl* / s_and* / v_readlane_b32 / v_writelane_b32; the kSym64 and
kBlockU256 instances (GEO = 1, 4) identical."""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_resources import code_objects

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
FP_OPCODE = re.compile(r"^v_\w*_(f16|f32|f64|bf16)(_|$)|^v_cvt_|^v_mfma_")


def kernels(path):
    out = {}
    for _, co in code_objects(open(path, "rb").read()):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co); f.flush()
            txt = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", f.name], capture_output=True, text=True).stdout
        name = None
        for line in txt.split("\n"):
            m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
            if m:
                name = m.group(1); out[name] = []
            elif name and line.strip():
                ins = re.sub(r"^\s*[0-9a-f]+:\s*", "", line.split("//")[0]).strip()
                ins = re.sub(r"<[^>]*\+0x[0-9a-f]+>", "<L>", ins)
                if ins and ins != "...":       # "...": objdump's mark for the zero padding up to the NEXT kernel's alignment --
                    out[name].append(ins)      # no instruction, and absent behind the last kernel of a code object
    for stream in out.values():                # the s_nop run the assembler pads the end of a text section with (instruction prefetch):
        end = max((i for i, ins in enumerate(stream) if ins.startswith(("s_endpgm", "s_branch", "s_cbranch"))), default=None)
        if end is not None and end + 1 < len(stream) and all(ins == "s_nop 0" for ins in stream[end + 1:]):
            del stream[end + 1:]               # only a run that is ALL s_nop behind the kernel's final s_endpgm / branch: never executed
    return out


def fp_only(stream):
    """The opcodes of the floating-point vector instructions of an instruction stream, spelling variants folded."""
    ops = (ins.split()[0] for ins in stream)
    ops = (re.sub(r"_(e32|e64)$", "", op).replace("v_fmac_", "v_fma_") for op in ops)
    return [op for op in ops if FP_OPCODE.match(op)]


STEP_KERNEL = re.compile(r"drone_kernelILi(\d)ELb(\d)ELi(\d)ELi(\d)ELb(\d)")
SCALAR_ADDRESS_OPCODE = re.compile(r"^(s_add|s_lshl|s_and)|^v_(read|write)lane_b32$")


def step_bound(a, b):
    """Verdict of --step-bound: the list of violations (empty: the bound holds), and a per-kernel report."""
    bad, changed, worst = [], 0, 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            bad.append(f"only in {'after' if name in b else 'before'}: {name[:100]}")
            continue
        x, y = a[name], b[name]
        if x == y:
            continue
        m = STEP_KERNEL.search(name)
        if not m:
            bad.append(f"not a step kernel, and different: {name[:100]}")
            continue
        short = "drone_kernel<K=%s,FAR=%s,MODE=%s,GEO=%s,EPI=%s>" % m.groups()
        if m.group(4) in ("1", "4"):
            bad.append(f"{short}: a kSym64 / kBlockU256 instance differs")
        if len(x) != len(y):
            bad.append(f"{short}: {len(x)} -> {len(y)} instructions")
            continue
        op = lambda ins: ins.split()[0]
        if collections.Counter(map(op, x)) != collections.Counter(map(op, y)):
            bad.append(f"{short}: the multiset of opcodes differs")
        lines = [(p, q) for p, q in zip(x, y) if p != q]
        other = sorted({o for p, q in lines for o in (op(p), op(q)) if not SCALAR_ADDRESS_OPCODE.match(o)})
        if other:
            bad.append(f"{short}: differing lines with other opcodes: {' '.join(other)}")
        changed += 1; worst = max(worst, len(lines))
        print(f"{short}: {len(x)} instructions, {len(lines)} differing lines ({' '.join(sorted({op(p) for p, _ in lines} | {op(q) for _, q in lines}))})")
    n_step = sum(1 for n in b if STEP_KERNEL.search(n))
    print(f"{len(b) - n_step} other kernels, {n_step} drone_kernel instances: {n_step - changed} identical, {changed} differ in at most {worst} lines")
    for line in bad:
        print("VIOLATION", line)
    print("step bound:", "HOLDS" if not bad else f"BROKEN ({len(bad)} violations)")
    return bad


def the_kernel(names, part, which):
    hits = [n for n in names if part in n]
    if len(hits) != 1:
        sys.exit(f"--pair: {part!r} matches {len(hits)} kernels of the {which} library, need exactly 1: {[h[:80] for h in hits]}")
    return hits[0]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--pair", action="append", default=[], metavar="OLD=NEW")
    ap.add_argument("--fp-only", action="store_true")
    ap.add_argument("--step-bound", action="store_true")
    args = ap.parse_args()
    a, b = kernels(args.before), kernels(args.after)
    if args.step_bound:
        return 1 if step_bound(a, b) else 0
    view = fp_only if args.fp_only else (lambda stream: stream)
    pairs = []
    for spec in args.pair:
        old, _, new = spec.partition("=")
        pairs.append((the_kernel(a, old, "first"), the_kernel(b, new, "second")))
    paired_a, paired_b = {o for o, _ in pairs}, {n for _, n in pairs}
    same = diff = 0
    for old, new in pairs:
        x, y = view(a[old]), view(b[new])
        if x != y:
            n = sum(p != q for p, q in zip(x, y)) + abs(len(x) - len(y))
            print(f"DIFFERENT ({len(x)} vs {len(y)} instructions, {n} differing lines)", old[:70], "->", new[:70]); diff += 1
        else:
            print(f"identical ({len(x)} instructions)", old[:70], "->", new[:70]); same += 1
    for name in sorted((set(a) - paired_a) | (set(b) - paired_b)):
        if name not in a or name not in b:
            print("only in", "after " if name in b else "before", name[:110]); diff += 1
        elif view(a[name]) != view(b[name]):
            x, y = view(a[name]), view(b[name])
            n = sum(p != q for p, q in zip(x, y)) + abs(len(x) - len(y))
            print(f"DIFFERENT ({len(x)} vs {len(y)} instructions, {n} differing lines)", name[:110]); diff += 1
        else:
            same += 1
    print(f"{same} kernels identical, {diff} different" + (" (floating-point opcode sequences)" if args.fp_only else ""))
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())
