#!/usr/bin/env python
"""Did a source change leave the generated gfx950 code alone? Compares the kernels of two sets of assembly dumps.

usage: isa_diff.py OLD.s NEW.s [NEW2.s ...]     (dumps from `hipcc --offload-arch=gfx950 ... --offload-device-only -S FILE.hip -o FILE.s`)

The NEW dumps are taken together (one translation unit split into several). Reported: kernels present on one side only; for every
common kernel whether its instruction stream and its kernel descriptor (.amdhsa_kernel block) are identical once what a change of
translation unit legitimately moves is normalised -- the function number in local labels (.LBB<n>_<m>, .Lfunc_end<n>, .Ltmp<n>),
comments, alignment directives -- and whether its amdhsa.kernels metadata is equal (register counts, LDS / scratch sizes, spill
counts, kernarg size, workgroup size). A unified diff is printed for the first kernel that differs. Exit status 0: identical."""
import difflib
import re
import sys

META_KEYS = [".agpr_count", ".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size", ".sgpr_spill_count",
             ".vgpr_spill_count", ".kernarg_segment_size", ".kernarg_segment_align", ".max_flat_workgroup_size", ".wavefront_size",
             ".uses_dynamic_stack"]


def normalise(lines):
    out = []
    for l in lines:
        l = l.split(";", 1)[0].strip()
        if not l or l.startswith((".p2align", ".align", ".balign")):
            continue
        l = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", l)
        l = re.sub(r"\.L(func_end|func_begin|tmp)\d+", r".L\1", l)
        out.append(re.sub(r"\s+", " ", l))
    return out


def kernels(path):
    """name -> (instructions, descriptor, metadata) for every kernel of one dump"""
    s = open(path).read()
    meta = {}
    if "amdhsa.kernels:" in s:
        for e in re.split(r"\n  - ", s[s.index("amdhsa.kernels:"):s.index("amdhsa.target:")])[1:]:
            name = re.search(r"\.name:\s*(\S+)", e).group(1)
            meta[name] = {k: m.group(1) for k in META_KEYS for m in [re.search(re.escape(k) + r":\s*(\S+)", e)] if m}
    out = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)^\s*\.end_amdhsa_kernel", s, re.M | re.S):
        name = m.group(1)
        a = s.index("\n" + name + ":") + 1
        body = s[a:s.index(".Lfunc_end", a)].split("\n")[1:]
        out[name] = (normalise(body), normalise(m.group(2).split("\n")), meta.get(name, {}))
    return out


def main(argv):
    if len(argv) < 3:
        print(__doc__)
        return 2
    old = kernels(argv[1])
    new = {}
    dup = []
    for p in argv[2:]:
        for name, k in kernels(p).items():
            if name in new:
                dup.append(name)
            new[name] = k
    bad = 0
    for what, names in (("only in " + argv[1], sorted(set(old) - set(new))), ("only in the new dumps", sorted(set(new) - set(old))),
                        ("in more than one new dump", dup)):
        print(f"{what}: {len(names)}")
        for n in names:
            print("   ", n)
        bad += len(names)
    first = None
    same = 0
    for name in sorted(set(old) & set(new)):
        (oi, od, om), (ni, nd, nm) = old[name], new[name]
        diffs = [w for w, a, b in (("instructions", oi, ni), ("descriptor", od, nd), ("metadata", om, nm)) if a != b]
        if diffs:
            bad += 1
            print(f"DIFFERENT ({', '.join(diffs)}): {name}")
            first = first or name
        else:
            same += 1
            print(f"identical  {len(oi):6d} lines  vgpr {om.get('.vgpr_count', '?'):>3} agpr {om.get('.agpr_count', '?'):>3} sgpr {om.get('.sgpr_count', '?'):>3}"
                  f"  lds {om.get('.group_segment_fixed_size', '?'):>6} scratch {om.get('.private_segment_fixed_size', '?'):>3}  {name}")
    print(f"{same} of {len(set(old) & set(new))} common kernels identical in instructions, descriptor and metadata")
    if first:
        (oi, od, om), (ni, nd, nm) = old[first], new[first]
        fmt = lambda i, d, m: i + ["-- descriptor"] + d + ["-- metadata"] + [f"{k}: {v}" for k, v in sorted(m.items())]
        print("\n".join(difflib.unified_diff(fmt(oi, od, om), fmt(ni, nd, nm), "old " + first, "new " + first, lineterm="", n=3)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
