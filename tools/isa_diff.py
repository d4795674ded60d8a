"""Which kernels differ between two gfx950 assembly listings of the product source.

usage: python tools/isa_diff.py BASE.s NEW.s        (tools/Makefile: make isa-diff BASE=<rev>)
(listings as for tools/isa_summary.py: hipcc --offload-arch=gfx950 -O3 -std=c++17
 --cuda-device-only -S ... sunsky_kernels.hip, with and without -DSS_XFORM_IDENTITY)

Per kernel label sunsky_*: the instruction and block-label lines from the label to its
.Lfunc_end, trailing ';' comments stripped and the local labels (.LBB<n>_<m>: n is the
function's position in the file) renamed to the ordinal of their first appearance, together
with the whole .amdhsa_kernel block (registers, LDS, scratch, kernarg size).  Prints one line
per kernel; for one that differs the instruction count and the VGPR / SGPR / LDS / scratch
figures of both sides.  Exits 1 if any kernel differs or is missing on either side.
"""
import re
import sys

FIGURES = (("vgpr", ".amdhsa_next_free_vgpr"), ("sgpr", ".amdhsa_next_free_sgpr"),
           ("lds", ".amdhsa_group_segment_fixed_size"), ("scratch", ".amdhsa_private_segment_fixed_size"))


def kernels(path):
    """name -> (normalised instruction lines, .amdhsa_kernel block lines)"""
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(sunsky_\w+):", text, re.M):
        body = text[m.end():text.index("\n.Lfunc_end", m.end())]
        k = body.index(".amdhsa_kernel " + m.group(1))
        meta = body[k:body.index(".end_amdhsa_kernel", k)].split()   # directive, value, directive, value, ...
        ordinal = {}
        ins = []
        for l in body[:k].splitlines():
            l = l.split(";")[0].strip()
            if l and (not l.startswith(".") or l.endswith(":")):
                ins.append(re.sub(r"\.L[A-Za-z]+\d+_\d+", lambda t: ordinal.setdefault(t.group(0), f".L{len(ordinal)}"), l))
        out[m.group(1)] = (ins, meta)
    return out


def figures(k):
    ins, meta = k
    vals = dict(zip(meta[0::2], meta[1::2]))
    n = sum(1 for l in ins if not l.endswith(":"))
    return f"{n} instructions  " + "  ".join(f"{short}={vals.get(key, '?')}" for short, key in FIGURES)


def main():
    base, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    for name in sorted(set(base) | set(new)):
        if name not in base or name not in new:
            print(f"MISSING   {name}: only in {sys.argv[2] if name in new else sys.argv[1]}")
        elif base[name] != new[name]:
            print(f"DIFFERS   {name}\n    base: {figures(base[name])}\n    new:  {figures(new[name])}")
        else:
            print(f"identical {name}")
            continue
        bad += 1
    print(f"{len(base)} kernels in {sys.argv[1]}, {len(new)} in {sys.argv[2]}: "
          + (f"{bad} differ or are missing" if bad else "all present and identical"))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
