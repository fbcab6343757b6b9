"""Which functions differ between two sets of gfx950 assembly files, wherever
they sit in their files.  Per function: the body (register names included)
with the assembler-local labels renumbered by first appearance, so that moving
a kernel inside a file or to another file changes nothing; per kernel also its
.amdhsa_kernel block (registers, LDS, scratch, kernarg size).  Prints the
functions that are missing, duplicated or different and exits non-zero if
there are any.  Not product code:
python tools/isa_funcdiff.py a.s [a2.s ...] -- b.s [b2.s ...]
(two files need no "--")."""
import re
import sys

LOCAL = re.compile(r"\.(LBB)\d+_\d+|\.(Lfunc_end|Lfunc_begin|Lpost_getpc|Ltmp|LJTI)\d+(?:_\d+)?")


def renumber(lines):
    seen = {}

    def sub(m):
        kind = m.group(1) or m.group(2)
        if m.group(0) not in seen:
            seen[m.group(0)] = f".{kind}#{len(seen)}"
        return seen[m.group(0)]

    return [LOCAL.sub(sub, l) for l in lines]


def code(l):
    """A line without its comment (comments name basic blocks by function index)."""
    return l.split(";", 1)[0].rstrip()


def funcs(paths):
    """name -> the function's definitions (renumbered body lines), and kernel
    name -> its .amdhsa_kernel blocks; one list entry per definition found."""
    out, desc = {}, {}
    for path in paths:
        cur = name = block = None
        for l in open(path):
            if block is not None:  # the descriptor sits between the code and .Lfunc_end
                if l.strip() == ".end_amdhsa_kernel":
                    block = None
                else:
                    block.append(code(l))
                continue
            m = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", l)
            if m:
                block = []
                desc.setdefault(m.group(1), []).append(block)
                continue
            m = re.match(r"^(_Z\w+):", l)
            if m and name is None:
                name, cur = m.group(1), []
            elif name is not None and l.startswith(".Lfunc_end"):
                out.setdefault(name, []).append(renumber(cur))
                name = None
            elif name is not None and code(l):
                cur.append(code(l))
    return out, desc


def main(argv):
    if "--" in argv:
        i = argv.index("--")
        left, right = argv[:i], argv[i + 1:]
    elif len(argv) == 2:
        left, right = argv[:1], argv[1:]
    else:
        sys.exit(__doc__)
    (a, ad), (b, bd) = funcs(left), funcs(right)
    bad = 0
    for n in sorted(set(a) | set(b)):
        what = None
        if n not in a or n not in b:
            what = "missing on the " + ("left" if n not in a else "right")
        elif len(a[n]) != 1 or len(b[n]) != 1 or len(ad.get(n, [])) > 1 or len(bd.get(n, [])) > 1:
            what = f"duplicated ({len(a[n])} / {len(b[n])} definitions)"
        elif a[n][0] != b[n][0]:
            what = f"body differs ({len(a[n][0])} -> {len(b[n][0])} lines)"
        elif ad.get(n) != bd.get(n):
            what = "kernel descriptor differs"
        if what:
            bad += 1
            print(f"{n[:110]}  {what}")
    kernels = len(set(ad) | set(bd))
    print(f"{len(set(a) | set(b))} functions ({kernels} kernels): {bad} missing, duplicated or different")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
