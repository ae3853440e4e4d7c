#!/usr/bin/env python3
"""Compare the device code of two `make asm` trees, kernel by kernel.

    python tools/asm_compare.py PARENT_BUILD CHANGE_BUILD

Each tree holds one UNIT.resources.txt (the remarks of -Rpass-analysis=kernel-resource-usage) and one UNIT.s per translation
unit.  Kernels are matched by name over all units together, so one that moved to another unit is compared with itself.  Printed:
the kernels per unit, the names on one side only, the names a side lists twice, the names whose resource figures differ, the names
that changed unit, and the number of kernels whose instruction text differs.  The text of a kernel is what stands between its
.type and its .size line, comments and .loc / .file / .cfi lines dropped, local labels renamed in order of appearance; whole
texts are compared.  The exit status is 0 when names, figures and texts all agree, else 1.
"""
import glob
import os
import re
import sys

FUNCTION = re.compile(r"remark: .*?Function Name: (\S+)")
FIGURE = re.compile(r"remark:\s+([A-Za-z][^:]*): (\S+)")
TYPE = re.compile(r"^\s*\.type\s+([^\s,]+),@function")
SIZE = re.compile(r"^\s*\.size\s+([^\s,]+),")
DROPPED = re.compile(r"^\s*\.(loc|file|cfi_\w+)\b")
LABEL = re.compile(r"\.L[A-Za-z_]\w*")


def read_resources(path):
    """[(name, {figure: value})] in the order of the file; a name the file lists twice appears twice."""
    out = []
    with open(path) as f:
        for line in f:
            m = FUNCTION.search(line)
            if m:
                out.append((m.group(1), {}))
                continue
            m = FIGURE.search(line)
            if m and out:
                out[-1][1][m.group(1).strip()] = m.group(2)
    return out


def normalise(lines):
    names = {}
    text = []
    for line in lines:
        line = line.split(";", 1)[0].rstrip()
        if not line.strip() or DROPPED.match(line):
            continue
        text.append(LABEL.sub(lambda m: names.setdefault(m.group(0), ".L%d" % len(names)), line))
    return "\n".join(text)


def read_listing(path):
    """{name: normalised text} of every function of the listing"""
    out, name, body = {}, None, []
    with open(path) as f:
        for line in f:
            if name is None:
                m = TYPE.match(line)
                if m:
                    name, body = m.group(1), []
                continue
            m = SIZE.match(line)
            if m and m.group(1) == name:
                out[name] = normalise(body)
                name = None
            else:
                body.append(line)
    return out


def read_tree(root):
    """{unit: [(name, figures)]}, {name: text}"""
    units, texts = {}, {}
    for res in sorted(glob.glob(os.path.join(root, "*.resources.txt"))):
        unit = os.path.basename(res)[: -len(".resources.txt")]
        units[unit] = read_resources(res)
        listing = os.path.join(root, unit + ".s")
        if os.path.exists(listing):
            kernels = {n for n, _ in units[unit]}
            texts.update({n: t for n, t in read_listing(listing).items() if n in kernels})
    return units, texts


def by_name(units):
    where, figures, twice = {}, {}, []
    for unit, kernels in units.items():
        for name, fig in kernels:
            if name in where:
                twice.append(name)
            where[name], figures[name] = unit, fig
    return where, figures, sorted(set(twice))


def compare(parent_root, change_root, out=sys.stdout):
    p_units, p_text = read_tree(parent_root)
    c_units, c_text = read_tree(change_root)
    p_where, p_fig, p_twice = by_name(p_units)
    c_where, c_fig, c_twice = by_name(c_units)

    def say(*a):
        print(*a, file=out)

    for unit in sorted(set(p_units) | set(c_units)):
        count = lambda u: "%4d" % len(u[unit]) if unit in u else "   -"
        say("%-13s parent %s kernels, change %s" % (unit, count(p_units), count(c_units)))
    say("parent names %d change names %d" % (len(p_where), len(c_where)))
    only_parent, only_change = sorted(set(p_where) - set(c_where)), sorted(set(c_where) - set(p_where))
    say("only at the parent:", only_parent)
    say("new on the change:", only_change)
    say("listed more than once at the parent:", p_twice)
    say("listed more than once on the change:", c_twice)
    both = sorted(set(p_where) & set(c_where))
    say("figures per remark:", sorted({len(f) for f in list(p_fig.values()) + list(c_fig.values())}),
        sorted({k for f in c_fig.values() for k in f}))
    figures_differ = [n for n in both if p_fig[n] != c_fig[n]]
    say("names whose figures differ: %d" % len(figures_differ))
    for n in figures_differ:
        say("   %s\n      parent %s\n      change %s" % (n, p_fig[n], c_fig[n]))
    moved = [n for n in both if p_where[n] != c_where[n]]
    say("names that changed unit: %d" % len(moved))
    for n in moved:
        say("   %s  %s -> %s  %s" % (n, p_where[n], c_where[n], c_fig[n]))
    no_text = [n for n in both if n not in p_text or n not in c_text]
    say("names without a listing on a side:", no_text)
    text_differs = [n for n in both if n not in no_text and p_text[n] != c_text[n]]
    say("kernels whose instruction text differs: %d of %d" % (len(text_differs), len(both) - len(no_text)))
    for n in text_differs:
        say("   %s (%d -> %d lines)\n      parent %s\n      change %s"
            % (n, p_text[n].count("\n") + 1, c_text[n].count("\n") + 1, p_fig[n], c_fig[n]))
    same = not (only_parent or only_change or p_twice or c_twice or figures_differ or no_text or text_differs)
    return 0 if same else 1


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(compare(sys.argv[1], sys.argv[2]))
