"""Is the generated code of the kernels what another commit's is?  No device needed.

    python tools/kernel_asm.py dump DIR [TREE]     device assembly of every source of build.SOURCES into DIR; TREE: a checkout
                                                   of another commit (default: this tree), compiled with its own build.FLAGS
    python tools/kernel_asm.py compare OLD NEW [A=B ...]
                                                   per kernel: instruction stream and .amdhsa_* descriptor, OLD against NEW;
                                                   A=B: a type that a kernel takes by value and that was renamed (its
                                                   name is part of the mangled name): A becomes B in OLD's text first

`compare` splits each file at the kernels' function labels, so that a kernel may move within its file, masks what only
numbers the functions of a file (.LBB<n>_, BB<n>_ in the loop comments and their padding, .Lfunc_end<n>) and the per-compilation __hip_cuid_<hex> symbol, and exits non-zero if a kernel of OLD is missing
from NEW or differs, or if a file without kernels differs at all.  Kernels that only NEW has are listed, not counted.
"""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK = [(re.compile(r"__hip_cuid_[0-9a-f]+"), "__hip_cuid_"), (re.compile(r"\.L([A-Za-z_]+?)\d+(?=_|\b)"), r".L\1"),
        # the loop comments name blocks without the .L, and stand in a column padded behind the numbered label
        (re.compile(r"\bBB\d+_(?=\d)"), "BB_"), (re.compile(r"[ \t]+;"), " ;")]


def dump(out, tree=ROOT):
    sys.path.insert(0, os.path.abspath(tree))
    from microaligner_amd import build
    build.build()   # writes build/ma_src_hash.h
    os.makedirs(out, exist_ok=True)
    cmds = [[build._hipcc()] + build.FLAGS + ["-I", os.path.join(build.HERE, "build"), "--offload-device-only", "-S",
             os.path.join(build.CSRC, s), "-o", os.path.join(out, s.replace(".hip", ".s"))] for s in build.SOURCES]
    with ThreadPoolExecutor(max_workers=8) as ex:
        for r in ex.map(lambda c: subprocess.run(c, capture_output=True, text=True), cmds):
            if r.returncode:
                sys.exit(r.stderr)


def kernels(path, renamed=()):
    """{mangled name: masked text from the kernel's .type line to its .Lfunc_end}, and the masked whole file"""
    text = open(path).read()
    for a, b in renamed:
        text = text.replace(a, b)
    for pat, to in MASK:
        text = pat.sub(to, text)
    names = re.findall(r"^\s*\.amdhsa_kernel (\S+)$", text, re.M)
    out = {}
    for n in names:
        a = text.index("\t.type\t%s,@function" % n)
        out[n] = text[a:text.index("\t.size\t%s, " % n, a)]
    return out, text


def compare(old, new, renamed=()):
    bad = 0
    for f in sorted(os.listdir(old)):
        if not os.path.exists(os.path.join(new, f)):
            print(f"{f}: missing in {new}")
            bad += 1
            continue
        (ko, to), (kn, tn) = kernels(os.path.join(old, f), renamed), kernels(os.path.join(new, f))
        diff = [n for n in ko if ko[n] != kn.get(n)]
        whole = "whole file identical" if to == tn else "file differs outside the kernels or in their order"
        if not ko and to != tn:
            diff.append("(no kernels)")
        print(f"{f}: {len(ko)} kernels, {len(ko) - len([n for n in diff if n in ko])} identical, "
              f"{len(set(kn) - set(ko))} new; {whole}")
        for n in diff:
            print("   DIFFERS" if n in kn or n == "(no kernels)" else "   MISSING", n)
        bad += len(diff)
    print(f"only in {new}:", sorted(set(os.listdir(new)) - set(os.listdir(old))))
    return bad


if __name__ == "__main__":
    if len(sys.argv) in (3, 4) and sys.argv[1] == "dump":
        dump(*sys.argv[2:])
    elif len(sys.argv) >= 4 and sys.argv[1] == "compare" and all(a.count("=") == 1 for a in sys.argv[4:]):
        sys.exit(1 if compare(sys.argv[2], sys.argv[3], [a.split("=") for a in sys.argv[4:]]) else 0)
    else:
        sys.exit(__doc__)
