#!/usr/bin/env python3
"""Instruction-level diff of two csrc trees: every unit that tools/resource_usage.py lists,
compiled to gfx950 assembly with the Makefile's flags from each tree, compared after dropping
what moves without the code moving (comment lines, directive and local-label lines, the per-unit
__hip_cuid_* label).  One row per unit: the number of differing lines (lines only in A plus lines
only in B); 0 means the two trees give that unit the same instruction stream.  For a refactor
that must not move a kernel: run it with the parent's tree (git archive) against the working tree.

usage: python tools/asm_diff.py CSRC_A CSRC_B [--exclude GLOB]... [-o OUT.txt]
(a unit's name is its source and its -D flags, e.g. "tmfwm_ragged_pre.hip -DTMF_B=8 -DTMF_RAGGED_PRE_PART=1")"""
import argparse
import fnmatch
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resource_usage as RU  # noqa: E402

FLAGS = [f for f in RU.FLAGS if f not in ("-Rpass-analysis=kernel-resource-usage", "-o", "/dev/null", "-c")] + ["-S"]


def strip_asm(text):
    """The lines of an assembly text that are code: no blank, comment (;) or directive / local
    label (.) lines, and no line that names the per-unit __hip_cuid_* symbol."""
    out = []
    for line in text.splitlines():
        s = line.strip()
        if s and s[0] not in ";." and "__hip_cuid_" not in s:
            out.append(s)
    return out


def differing_lines(a_text, b_text):
    """Lines only in A plus lines only in B, of the two stripped texts (diff's count)."""
    a, b = strip_asm(a_text), strip_asm(b_text)
    if a == b:
        return 0
    with tempfile.TemporaryDirectory() as d:
        for name, lines in (("a", a), ("b", b)):
            with open(os.path.join(d, name), "w") as f:
                f.writelines(line + "\n" for line in lines)
        r = subprocess.run(["diff", os.path.join(d, "a"), os.path.join(d, "b")], capture_output=True, text=True)
    return sum(1 for line in r.stdout.splitlines() if line[:1] in "<>")


def unit_name(tu, extra):
    return " ".join([tu] + [f for f in extra if f.startswith("-D")])


def assembly(csrc, tu, extra):
    pre = [f for f in extra if f in ("-x", "hip")]
    post = [f for f in extra if f not in pre]
    r = subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + ["-o", "-"] + pre + [tu] + post, cwd=csrc, capture_output=True, text=True)
    if r.returncode:
        sys.stderr.write(r.stderr[-3000:])
        raise SystemExit(f"{csrc}: {unit_name(tu, extra)}: compile failed")
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("csrc_a")
    ap.add_argument("csrc_b")
    ap.add_argument("--exclude", action="append", default=[], help="glob over unit names; may repeat")
    ap.add_argument("-o", "--out")
    a = ap.parse_args()
    units = RU.units(a.csrc_b)
    if [unit_name(*u) for u in RU.units(a.csrc_a)] != [unit_name(*u) for u in units]:
        raise SystemExit("the two trees list different units")
    units = [u for u in units if not any(fnmatch.fnmatch(unit_name(*u), g) for g in a.exclude)]

    def one(u):
        return differing_lines(assembly(a.csrc_a, *u), assembly(a.csrc_b, *u))

    with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
        counts = list(ex.map(one, units))
    rows = ["# unit | differing lines"] + ["%s | %d" % (unit_name(*u), n) for u, n in zip(units, counts)]
    rows.append("# %d units, %d identical" % (len(units), sum(1 for n in counts if n == 0)))
    text = "\n".join(rows) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
