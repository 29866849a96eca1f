#!/usr/bin/env python3
"""Kernel by kernel, two device assemblies of geo_render.hip (tools/isa.sh):

    python3 tools/isa_compare.py OLD.s NEW.s [TABLE]

TABLE: lines "old_symbol new_symbol" for the kernels that were renamed (the
others keep their symbol).  Per kernel, in OLD's order: instruction count,
next_free_vgpr, next_free_sgpr, accum_offset, scratch, LDS and kernarg size of
both, the differing lines once the kernel's own symbol and the numbers of its
local labels are normalised, and how many of those are anything else than the
immediate offset of a scalar load or .amdhsa_kernarg_size (an argument that
moved).  Then the kernels whose position differs, and the totals."""
import difflib
import re
import sys

FIELDS = (("vgpr", "next_free_vgpr"), ("sgpr", "next_free_sgpr"), ("accum", "accum_offset"),
          ("scratch", "private_segment_fixed_size"), ("lds", "group_segment_fixed_size"), ("kernarg", "kernarg_size"))
INSN = re.compile(r"^\s+(s|v|ds|buffer|global|flat|scratch)_\w+")


def kernels(path):
    """[(symbol, lines from its label to the end of its function: code, descriptor, resource records)] in the file's order."""
    lines = open(path).read().split("\n")
    names = [m.group(1) for l in lines if (m := re.match(r"\s*\.amdhsa_kernel (\S+)", l))]
    start = {m.group(1): i for i, l in enumerate(lines) if (m := re.match(r"(\w+):\s+; @\1$", l))}
    out = []
    for n in names:
        end = next(i for i in range(start[n], len(lines)) if "; -- End function" in lines[i])
        out.append((n, lines[start[n]:end + 1]))
    return out


def normal(sym, body, loose):
    out = []
    for l in body:
        l = l.replace(sym, "KERNEL")
        l = re.sub(r"\.L(BB|func_end|func_begin|tmp)\d+", r".L\1", l)
        if loose:
            l = re.sub(r"^(\s+s_load_dword\w*\s+[^,]+,\s*s\[\d+:\d+\],) 0x[0-9a-f]+", r"\1 OFF", l)
            l = re.sub(r"(\.amdhsa_kernarg_size) \d+", r"\1 N", l)
        out.append(l)
    return out


def differing(a, b):
    return sum(1 for l in difflib.unified_diff(a, b, lineterm="", n=0) if l[:1] in "+-" and l[:3] not in ("+++", "---"))


def stats(body):
    s = {"insts": sum(1 for l in body if INSN.match(l))}
    for key, field in FIELDS:
        s[key] = next(int(l.split()[-1]) for l in body if f".amdhsa_{field} " in l)
    return s


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    table = dict(l.split() for l in open(sys.argv[3]) if l.strip()) if len(sys.argv) > 3 else {}
    new_at = {n: i for i, (n, _) in enumerate(new)}
    cols = ["insts"] + [k for k, _ in FIELDS]
    print("#   " + " ".join(f"{c:>11}" for c in cols) + "  lines  other  kernel (old -> new)")
    moved, total, total_other, changed = [], 0, 0, 0
    for i, (sym, body) in enumerate(old):
        nsym = table.get(sym, sym)
        if nsym not in new_at:
            print(f"{i + 1:<3} missing in NEW: {sym} -> {nsym}")
            continue
        nbody = new[new_at[nsym]][1]
        if new_at[nsym] != i:
            moved.append((sym, i + 1, new_at[nsym] + 1))
        a, b = stats(body), stats(nbody)
        d = differing(normal(sym, body, False), normal(nsym, nbody, False))
        o = differing(normal(sym, body, True), normal(nsym, nbody, True))
        total, total_other, changed = total + d, total_other + o, changed + (d > 0)
        name = sym if nsym == sym else f"{sym} -> {nsym}"
        print(f"{i + 1:<3} " + " ".join(f"{str(a[c]) + '/' + str(b[c]):>11}" for c in cols) + f"  {d:5d}  {o:5d}  {name}")
    extra = [n for n, _ in new if n not in {table.get(s, s) for s, _ in old}]
    print(f"kernels: {len(old)} old, {len(new)} new; not in OLD: {extra}; position differs: {moved}")
    print(f"differing lines: {total} in {changed} kernels; other than a scalar load's offset or the kernarg size: "
          f"{total_other}")
    same = all(stats(b)[c] == stats(new[new_at[table.get(s, s)]][1])[c] for s, b in old if table.get(s, s) in new_at
               for c in cols if c != "kernarg")
    print("instruction, register, scratch and LDS counts: " + ("all equal" if same else "DIFFER"))


if __name__ == "__main__":
    main()
