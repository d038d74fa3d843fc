#!/usr/bin/env python3
"""Developer tool (no GPU needed): did a change move the device code? Compiles every csrc/*.hip and unit/*.hip of two source trees to
gfx950 assembly with the product's flags (check_codegen.makefile_flags()), splits the assembly into functions, and compares each
function's text after dropping what carries no code: comments, directives, and the numbers of block and temporary labels.

usage: tools/codegen_diff.py OLD_TREE NEW_TREE        (two checkouts of this repository)
Prints one line per function of either tree:
    SAME | DIFF | OLD_ONLY | NEW_ONLY   instruction lines old   new   file: function
(a function that moved between files is matched by its name and listed under its new file, `<- old file` behind it), and exits 1 when
a function present in both trees differs. The comparison is of text alone: the tool looks for no instruction in particular."""
import glob, os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor

import check_codegen

LOCAL_LABEL = re.compile(r"\.L[A-Za-z_]*\d+(?:_\d+)*")


def split_functions(text):
    """{function: [lines]} of one assembly listing: from `name:  ; @name` to the function's end label, comments and blank lines gone,
    directives gone, every local label (.LBB3_12, .Ltmp7, .LJTI3_0 ...) renamed by order of first appearance in the function."""
    out, name, body, names = {}, None, None, None
    for raw in text.split("\n"):
        if name is None:
            m = re.match(r"([A-Za-z_$][\w$.]*):\s*;\s*@", raw)
            if m:
                name, body, names = m.group(1), [], {}
            continue
        line = raw.split(";", 1)[0].rstrip()
        if re.match(r"\.Lfunc_end\d+:", line):
            out[name], name = body, None
            continue
        if not line.strip():
            continue
        if re.match(r"\s*\.", line) and not re.match(r"\.L[\w$]*:", line):
            continue  # a directive: alignment, cfi, sections, sizes
        line = LOCAL_LABEL.sub(lambda m: names.setdefault(m.group(0), ".L%d" % len(names)), line)
        body.append((" " if line[0].isspace() else "") + " ".join(line.split()))  # (instructions stay indented, labels do not)
    return out


def instruction_lines(body):
    """as tools/check_codegen.py counts them: indented lines that begin with a mnemonic"""
    return sum(1 for l in body if re.match(r"\s+[a-z]", l))


def compare(old, new):
    """old, new: {file: {function: body}}. Returns [(status, n_old, n_new, file, function, moved_from)], sorted by file and function."""
    where = {}
    for side, tree in enumerate((old, new)):
        for f, funcs in tree.items():
            for fn in funcs:
                where.setdefault(fn, ([], []))[side].append(f)
    rows = []
    for fn, (fo, fnw) in where.items():
        pairs = [(f, f) for f in fo if f in fnw]
        lo, ln = [f for f in fo if f not in fnw], [f for f in fnw if f not in fo]
        if len(lo) == 1 and len(ln) == 1:  # one definition left on either side: the function moved
            pairs.append((lo.pop(), ln.pop()))
        for a, b in pairs:
            same = old[a][fn] == new[b][fn]
            rows.append(("SAME" if same else "DIFF", instruction_lines(old[a][fn]), instruction_lines(new[b][fn]), b, fn, a if a != b else None))
        rows += [("OLD_ONLY", instruction_lines(old[a][fn]), None, a, fn, None) for a in lo]
        rows += [("NEW_ONLY", None, instruction_lines(new[b][fn]), b, fn, None) for b in ln]
    return sorted(rows, key=lambda r: (r[3], r[4]))


def assembly(tree, rel):
    pkg = os.path.join(tree, "yocto-hair_amd")
    with tempfile.NamedTemporaryFile(suffix=".s") as f:
        subprocess.run([check_codegen.hipcc(), *check_codegen.makefile_flags(), "--cuda-device-only", "-S", "-I" + os.path.join(tree, "include"),
                        "-I" + os.path.join(pkg, "csrc"), os.path.join(pkg, rel), "-o", f.name], check=True, stderr=subprocess.DEVNULL)
        return split_functions(open(f.name).read())


def sources(tree):
    pkg = os.path.join(tree, "yocto-hair_amd")
    return sorted(os.path.relpath(p, pkg) for d in ("csrc", "unit") for p in glob.glob(os.path.join(pkg, d, "*.hip")))


def main(argv):
    if len(argv) != 3:
        raise SystemExit(__doc__)
    jobs = [(side, rel) for side in (0, 1) for rel in sources(argv[1 + side])]
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:  # the threads only wait for their compiler
        done = list(pool.map(lambda j: assembly(argv[1 + j[0]], j[1]), jobs))
    trees = ({}, {})
    for (side, rel), funcs in zip(jobs, done):
        trees[side][rel] = funcs
    rows = compare(*trees)
    for status, n_old, n_new, f, fn, moved in rows:
        count = lambda n: "     -" if n is None else "%6d" % n
        print("%-8s %s %s  %s: %s%s" % (status, count(n_old), count(n_new), f, fn, "   <- " + moved if moved else ""))
    return 1 if any(r[0] == "DIFF" for r in rows) else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
