#!/usr/bin/env python3
"""Resource-usage listing of every gfx950 kernel of thatsmyface_amd/csrc (the compiler's
kernel-resource-usage remarks, the Makefile's flags), one row per kernel, sorted by name:
the form of profiles/*_resource_usage_{before,after}.txt.  Two listings of two trees compare
with diff; tools/regs.py is the short interactive form for the embed / extract kernels.

usage: python tools/resource_usage.py OUT.txt [CSRC_DIR]"""
import glob
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize",
         "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-o", "/dev/null", "-c"]
ILP = ["-mllvm", "-amdgpu-sched-strategy=max-ilp"]
SIZES = (4, 6, 8, 10, 12, 14, 16)
# compiled once per block size with -DTMF_B=<b> (the Makefile's PER_SIZE)
PER_SIZE = ("tmfwm_fixup.hip", "tmfwm_ragged_fixup.hip", "tmfwm_keyed_fixup.hip", "tmfwm_ragged_strip.hip", "tmfwm_embed_key.hip",
            "tmfwm_ragged_pre.hip")
ALPHAS = ("tmfwm_ragged_strip.hip", "tmfwm_ragged_fixup.hip", "tmfwm_ragged_pre.hip")
KEYS = ["TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill",
        "LDS Size [bytes/block]"]


def units(csrc):
    out = []
    for path in sorted(glob.glob(os.path.join(csrc, "*.hip"))):
        tu = os.path.basename(path)
        if tu in PER_SIZE:
            mine = []  # this source's objects
            for b in SIZES:
                if (tu, b) == ("tmfwm_ragged_strip.hip", 8):  # two objects: embed / extract under max-ILP, the keyed kernels not
                    mine += [(tu, ["-DTMF_B=8", "-DTMF_RAGGED_PART=1"] + ILP), (tu, ["-DTMF_B=8", "-DTMF_RAGGED_PART=2"])]
                elif (tu, b) == ("tmfwm_ragged_pre.hip", 8):  # two objects: the pre-pass, and the list pass under max-ILP
                    mine += [(tu, ["-DTMF_B=8", "-DTMF_RAGGED_PRE_PART=1"]), (tu, ["-DTMF_B=8", "-DTMF_RAGGED_PRE_PART=2"] + ILP)]
                elif (tu, b) == ("tmfwm_embed_key.hip", 8):  # under max-ILP, as embed_kernel<8>
                    mine.append((tu, ["-DTMF_B=8"] + ILP))
                else:
                    mine.append((tu, ["-DTMF_B=%d" % b]))
            if tu in ALPHAS:  # each object once more as the per-frame form (the Makefile's ALPHA_OBJS), built as its sibling
                mine += [(t, f + ["-DTMF_RAGGED_ALPHAS=1"]) for t, f in mine]
            out += mine
        else:
            out.append((tu, ILP if tu == "tmfwm_embed8.hip" else []))
    return out + [("tmfwm_capi.cpp", ["-x", "hip"]), ("tmfwm_multi.cpp", ["-x", "hip"])]


def remarks(csrc, tu, extra):
    pre = [f for f in extra if f in ("-x", "hip")]
    post = [f for f in extra if f not in pre]
    r = subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + pre + [tu] + post, cwd=csrc, capture_output=True, text=True)
    if r.returncode:
        sys.stderr.write(r.stderr[-3000:])
        raise SystemExit(f"{tu}: compile failed")
    return r.stderr


def main():
    out_path = sys.argv[1]
    csrc = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "thatsmyface_amd", "csrc")
    with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
        outs = list(ex.map(lambda u: remarks(csrc, *u), units(csrc)))
    rows = {}
    for text in outs:
        cur = None
        for line in text.splitlines():
            m = re.search(r"remark: +([A-Za-z ]+(?:\[[^\]]+\])?): (\S+)", line)
            if not m:
                continue
            k, v = m.group(1).strip(), m.group(2)
            if k == "Function Name":
                name = subprocess.run(["c++filt", v], capture_output=True, text=True).stdout.strip() or v
                cur = rows.setdefault(re.sub(r"\(.*$", "", name), {})
            elif cur is not None and k in KEYS:
                cur[k] = v
    with open(out_path, "w") as f:
        f.write("# kernel | TotalSGPRs | VGPRs | AGPRs | ScratchSize | Occupancy | SGPRs Spill | VGPRs Spill | LDS Size\n")
        for n in sorted(rows):
            f.write(n + " | " + " | ".join(rows[n].get(k, "?") for k in KEYS) + "\n")
    print(len(rows), "kernels ->", out_path)


if __name__ == "__main__":
    main()
