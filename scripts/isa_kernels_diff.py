"""Kernel-by-kernel comparison of two device-assembly dumps (scripts/isa_dump.sh):
    python scripts/isa_kernels_diff.py DIR_A DIR_B [--renamed-ok]
Every *.clean.s of each directory is cut into kernels — the code from the symbol's label to its .Lfunc_end, plus its
.amdhsa_kernel descriptor block — and the two sets are compared by symbol name, whichever file a kernel came from and in
whatever order. Reports kernels missing from DIR_B, added in DIR_B, or textually different, and exits 1 on any of them
(0: same kernels, same code). A kernel compiled into several files of one directory (a template instantiated in two
translation units) must be the same in each.
--renamed-ok: a kernel missing under one symbol and added under another with the same bare function name and identical
code (one that moved into or out of a namespace, or whose template gained a defaulted argument) is listed as renamed, not
as a difference; of several added symbols with that name, the one with the identical code is its twin."""
import glob
import os
import re
import sys


def kernels(directory):
    """{symbol: text} over every *.clean.s of the directory; local label numbers are per file, so they are dropped."""
    out, clash = {}, []
    for path in sorted(glob.glob(os.path.join(directory, "*.clean.s"))):
        lines = open(path).read().split("\n")
        names = {m.group(1) for l in lines for m in [re.match(r"\s*\.amdhsa_kernel (\S+)", l)] if m}
        body, desc, cur, cur_desc = {}, {}, None, None
        for l in lines:
            if cur is None and l.endswith(":") and l[:-1] in names:
                cur = l[:-1]
                body[cur] = []
            if cur is not None:
                body[cur].append(re.sub(r"\.L(func_end|tmp|JTI|func_begin)\d+(_\d+)?", r".L\1", l))
                if re.match(r"\.Lfunc_end\d+:", l):
                    cur = None
            # (the descriptor block may sit inside the code's span, in its own section: it is kept either way)
            m = re.match(r"\s*\.amdhsa_kernel (\S+)", l)
            if m:
                cur_desc = m.group(1)
                desc[cur_desc] = []
            if cur_desc is not None:
                desc[cur_desc].append(l)
                if re.match(r"\s*\.end_amdhsa_kernel", l):
                    cur_desc = None
        for n in sorted(names):
            if n not in body:
                sys.exit(f"{path}: kernel {n} has a descriptor but no code")
            text = "\n".join(body[n] + desc[n])
            if n in out and out[n] != text:
                clash.append(n)
            out[n] = text
    return out, clash


def bare(symbol):
    """The function's own identifier of an Itanium-mangled nested name (_ZN3fcr12_GLOBAL__N_13fooE... -> foo)."""
    m, last = re.match(r"_ZN?", symbol), symbol
    i = m.end() if m else 0
    while True:
        d = re.match(r"\d+", symbol[i:])
        if not d:
            return last
        n = int(d.group())
        last = symbol[i + len(d.group()):i + len(d.group()) + n]
        i += len(d.group()) + n


def main(argv):
    renamed_ok = "--renamed-ok" in argv
    dirs = [a for a in argv if not a.startswith("--")]
    if len(dirs) != 2:
        sys.exit(__doc__)
    (a, clash_a), (b, clash_b) = kernels(dirs[0]), kernels(dirs[1])
    if not a or not b:
        sys.exit("no kernels found: run scripts/isa_dump.sh into both directories first")
    missing, added = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    differ = sorted(n for n in set(a) & set(b) if a[n] != b[n])
    renamed = []
    for n in list(missing):
        twins = [m for m in added if bare(m) == bare(n) and a[n].replace(n, "@") == b[m].replace(m, "@")]
        if len(twins) == 1:
            renamed.append((n, twins[0]))
            missing.remove(n)
            added.remove(twins[0])
    for title, names in (("differs between files of " + dirs[0], clash_a), ("differs between files of " + dirs[1], clash_b),
                         ("missing from " + dirs[1], missing), ("added in " + dirs[1], added), ("different code", differ)):
        for n in names:
            print(f"{title}: {n}")
    for old, new in renamed:
        print(f"renamed, same code: {old} -> {new}")
    bad = len(clash_a) + len(clash_b) + len(missing) + len(added) + len(differ) + (0 if renamed_ok else len(renamed))
    print(f"{len(a)} kernels in {dirs[0]}, {len(b)} in {dirs[1]}: {len(missing)} missing, {len(added)} added, "
          f"{len(differ)} different, {len(renamed)} renamed")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
