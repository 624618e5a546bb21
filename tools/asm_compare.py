"""Compares two sets of device assembly listings (`make -C
wasm-pathtracer_amd/csrc asm` gives build/wpt_render.s and build/wpt_post.s)
function by function: the instructions, the kernel descriptor and the register
counts of every function of the first set must be in the second unchanged.
Either side is one listing or several, which together must hold each function
once (a kernel that moved from one unit to another is then compared like any
other). Block and function label numbers, which shift when a function is added,
are ignored. Prints the functions only the second set has; exit 1 on a
difference, a missing function or one that a side holds twice.
Usage: python3 tools/asm_compare.py PARENT.s NEW.s
       python3 tools/asm_compare.py PARENT.s [...] -- NEW_A.s NEW_B.s [...]"""
import re
import sys


def functions(path):
    txt = open(path).read()
    chunks = re.split(r"^\.Lfunc_end\d+:\n", txt, flags=re.M)
    out = {}
    for i, c in enumerate(chunks[:-1]):
        name = re.findall(r"^(_Z\w+):", c, re.M)[-1]
        body = c[c.rindex("\n" + name + ":"):]
        # the resource counts (.set NAME.num_vgpr ...) follow the end label
        meta = "\n".join(l for l in chunks[i + 1].split("\n")[:40] if l.startswith("\t.set " + name + "."))
        out[name] = body + meta
    return out


def side(paths):
    """The functions of several listings, and the names more than one holds."""
    out, twice = {}, []
    for p in paths:
        for name, body in functions(p).items():
            if name in out:
                twice.append(name)
            out[name] = body
    return out, twice


def norm(body):
    body = re.sub(r"\.LBB\d+_", ".LBB_", body)
    # the loop comments name blocks too, and their column follows the label's
    # length (a function number going from two digits to three)
    body = re.sub(r"\bBB\d+_", "BB_", body)
    body = re.sub(r"[ \t]+;", " ;", body)
    body = re.sub(r"\.Lfunc_(begin|end)\d+", ".Lfunc_", body)
    return re.sub(r"\.Ltmp\d+", ".Ltmp", body)


def main():
    args = sys.argv[1:]
    if "--" in args:
        first, second = args[:args.index("--")], args[args.index("--") + 1:]
    else:
        first, second = args[:1], args[1:]
    if not first or not second:
        sys.exit(__doc__)
    (a, twice_a), (b, twice_b) = side(first), side(second)
    missing = [k for k in a if k not in b]
    differ = [k for k in a if k in b and norm(a[k]) != norm(b[k])]
    lines = sum(len(v.splitlines()) for v in a.values())
    print(f"functions: first {len(a)} ({lines} lines), second {len(b)}; identical {len(a) - len(missing) - len(differ)}, "
          f"different {len(differ)}, missing {len(missing)}, twice in a side {len(twice_a) + len(twice_b)}")
    for k in differ:
        print("DIFFERS", k)
    for k in missing:
        print("MISSING", k)
    for k in twice_a:
        print("TWICE in first:", k)
    for k in twice_b:
        print("TWICE in second:", k)
    for k in b:
        if k not in a:
            print("only in second:", k)
    return 1 if differ or missing or twice_a or twice_b else 0


if __name__ == "__main__":
    sys.exit(main())
