#!/usr/bin/env python3
"""Compare the gfx950 machine code of two builds of thatsmyface_amd/csrc, object by object: the
.text section of each object's gfx950 code object (unbundled as tools/kernel_ids.py does it, then
llvm-objcopy -O binary --only-section=.text) and the kernel ids of tools/kernel_ids.py.
usage: compare_text.py PARENT_CSRC CHANGE_CSRC > text_compare.txt"""
import glob
import hashlib
import os
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tools"))
import kernel_ids  # noqa: E402


def text_of(obj):
    with tempfile.TemporaryDirectory() as d:
        try:
            co, _ = kernel_ids.code_object(obj, d)
        except subprocess.CalledProcessError:
            return None  # host-only object
        out = os.path.join(d, "text.bin")
        subprocess.run([f"{kernel_ids.LLVM}/llvm-objcopy", "-O", "binary", "--only-section=.text", co, out], check=True)
        with open(out, "rb") as f:
            return f.read()


def main():
    parent, change = sys.argv[1:3]
    names = sorted({os.path.basename(p) for d in (parent, change) for p in glob.glob(os.path.join(d, "*.o"))})
    bad = 0
    print("# object | .text bytes parent / change | sha256[:16] parent / change | .text | kernel ids")
    for n in names:
        a, b = os.path.join(parent, n), os.path.join(change, n)
        if not (os.path.exists(a) and os.path.exists(b)):
            print(f"{n} | only in {'parent' if os.path.exists(a) else 'change'}")
            continue
        ta, tb = text_of(a), text_of(b)
        if ta is None or tb is None:
            continue
        ids = "equal" if kernel_ids.tu_kernels(a) == kernel_ids.tu_kernels(b) else "DIFFER"
        same = "equal" if ta == tb else "DIFFER"
        bad += same != "equal" or ids != "equal"
        print(f"{n} | {len(ta)} / {len(tb)} | {hashlib.sha256(ta).hexdigest()[:16]} / {hashlib.sha256(tb).hexdigest()[:16]} | {same} | {ids}")
    print(f"# {bad} object(s) differ")


if __name__ == "__main__":
    main()
