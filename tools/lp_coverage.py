#!/usr/bin/env python3
"""Which lines and branch directions of the dgesdd route's restatement (oracle/tmfwm_lapack.c,
which thatsmyface_amd/csrc/tmfwm_lapack.h mirrors routine by routine) the test corpora reach.

Copies the oracle's sources to a temporary directory, builds them there with tmfwm_lapack.c
under `gcc --coverage -O0`, runs each corpus of tests/lp_corpus.py through the library in a child
process and reads `gcov -b`.  Nothing is written into oracle/_build or the tree (except --json's
file, if asked for).

Corpora:
  covers       the cover classes and noise frame of the GPU tests, embed + extract, lapack route
  patterns     lp_corpus.pattern_cover, embed + extract (alpha 0.1, 1.0, -0.5), lapack route
  matrices     lp_corpus.matrices through the stage entry point (lp_svd_blocks)
  bidiagonals  lp_corpus.bidiagonals through the stage entry point

With hipcc present it also builds tests/native/lp_host.cpp (the device header compiled for the
host) under `hipcc --cuda-host-only --coverage -O0`, whose notes this gcov reads, and reports the
header's own lines.

    python tools/lp_coverage.py [--json OUT.json] [--noise-size HxW] [--unreached] [--no-header]
"""
from __future__ import annotations

import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE = os.path.join(ROOT, "oracle")
CORPORA = ("covers", "patterns", "matrices", "bidiagonals")
SRC = "tmfwm_lapack.c"
CFLAGS = ["-fPIC", "-fopenmp", "-ffp-contract=off", "-fno-fast-math", "-Wall"]


def available() -> bool:
    return bool(shutil.which("gcov") and shutil.which("gcc") and shutil.which("g++"))


def build(tmp: str) -> str:
    """The oracle library in tmp, tmfwm_lapack.c instrumented; returns the .so path."""
    for f in os.listdir(ORACLE):
        if f.endswith((".c", ".cpp", ".h")):
            shutil.copy(os.path.join(ORACLE, f), tmp)
    run = lambda cmd: subprocess.run(cmd, cwd=tmp, check=True)  # noqa: E731
    run(["gcc", "--coverage", "-fprofile-update=atomic", "-O0", "-std=c11", *CFLAGS, "-c", SRC, "-o", "tmfwm_lapack.o"])
    run(["gcc", "-O2", "-std=c11", *CFLAGS, "-c", "tmfwm_oracle.c", "-o", "tmfwm_oracle.o"])
    run(["g++", "-O2", "-std=c++17", *CFLAGS, "-c", "tmfwm_cert.cpp", "-o", "tmfwm_cert.o"])
    so = os.path.join(tmp, "libtmfwm_oracle_cov.so")
    run(["g++", "-shared", "-fopenmp", "--coverage", "-o", so, "tmfwm_lapack.o", "tmfwm_oracle.o", "tmfwm_cert.o", "-lm"])
    return so


# ------------------------------------------------------------------------------------------------
# child process: one corpus through the instrumented library
# ------------------------------------------------------------------------------------------------
def child(corpus: str, so: str, noise_hw) -> None:
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import lp_corpus as C
    from oracle import oracle as O

    O._LIB_PATH = so  # the instrumented copy; never (re)build the tree's own
    O.build = lambda force=False: so
    for b in C.ALL_B:
        if corpus in ("matrices", "bidiagonals"):
            O.lp_svd_blocks(getattr(C, corpus)(b, 0)[0], nthreads=1)
            continue
        if corpus == "covers":
            jobs = [(c, t, (0.1,)) for c, t in C.cover_standin(b, noise_hw)]
        else:
            c, _ = C.pattern_cover(b)
            jobs = [(c, C.pattern_tile(c.shape[0] // b, c.shape[1] // b), (0.1, 1.0, -0.5))]
        for c, t, alphas in jobs:
            for alpha in alphas:
                e = O.embed_frame(c, t, b, alpha, nthreads=1, route="lapack")
                O.extract_frame(e, c, b, alpha, nthreads=1, route="lapack")


# ------------------------------------------------------------------------------------------------
# gcov
# ------------------------------------------------------------------------------------------------
_LINE = re.compile(r"^\s*([^:]+):\s*(\d+):(.*)$")
_FUNC = re.compile(r"^function (\S+) called (\d+)")
_BRANCH = re.compile(r"^branch\s+\d+ (taken (\d+)|never executed)")


def read_gcov(tmp: str) -> dict:
    """{routine: {"lines": {lineno: (text, hit)}, "branches": {(lineno, k): taken}}} from gcov -b."""
    subprocess.run(["gcov", "-b", "-c", "-o", tmp, SRC], cwd=tmp, check=True, stdout=subprocess.DEVNULL)
    out: dict = {}
    fn, ln, k = None, 0, 0
    with open(os.path.join(tmp, SRC + ".gcov")) as f:
        for raw in f:
            m = _FUNC.match(raw)
            if m:
                fn = m.group(1)
                out.setdefault(fn, {"lines": {}, "branches": {}})
                continue
            m = _BRANCH.match(raw)
            if m:
                if fn is not None:
                    out[fn]["branches"][(ln, k)] = bool(m.group(2) and int(m.group(2)) > 0)
                k += 1
                continue
            m = _LINE.match(raw)
            if not m:
                continue  # "call" lines, the per-function summaries
            cnt, ln, text, k = m.group(1).strip(), int(m.group(2)), m.group(3), 0
            if cnt == "-" or fn is None:
                continue
            out[fn]["lines"][ln] = (text.strip(), cnt not in ("#####", "=====") and not cnt.startswith("0"))
    return out


def measure(noise_hw=(1080, 1920), corpora=CORPORA) -> dict:
    """{corpus: read_gcov() result} -- each corpus run alone from zeroed counters."""
    res = {}
    with tempfile.TemporaryDirectory(prefix="lp_coverage_") as tmp:
        so = build(tmp)
        env = dict(os.environ, OMP_NUM_THREADS="1")
        for corpus in corpora:
            for f in os.listdir(tmp):
                if f.endswith(".gcda"):
                    os.remove(os.path.join(tmp, f))
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", corpus, "--so", so,
                            "--noise-size", "%dx%d" % noise_hw], check=True, env=env, cwd=tmp)
            res[corpus] = read_gcov(tmp)
    return res


# ------------------------------------------------------------------------------------------------
# the device header itself, compiled for the host (tests/native/lp_host.cpp)
# ------------------------------------------------------------------------------------------------
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
HDR = "tmfwm_lapack.h"


def header_available() -> bool:
    return available() and (os.path.exists(HIPCC) or bool(shutil.which("hipcc")))


def header_child(so: str) -> None:
    """matrices, bidiagonals and the DCT blocks of the pattern covers (original and watermarked)
    through the host build: both lane policies, with vectors and S only."""
    import ctypes

    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import lp_corpus as C
    import numpy as np
    from lapack_path import _blocks
    from oracle import oracle as O

    L = ctypes.CDLL(so)
    vp = ctypes.c_void_p
    L.lp_host_svd_blocks.argtypes = [vp, ctypes.c_longlong, ctypes.c_int, vp, vp, vp, ctypes.c_int, ctypes.c_int]
    for b in C.ALL_B:
        cov, _ = C.pattern_cover(b)
        emb = O.embed_frame(cov, C.pattern_tile(cov.shape[0] // b, cov.shape[1] // b), b, 0.1, route="lapack")
        D = np.concatenate([C.matrices(b)[0], C.bidiagonals(b)[0]] +
                           [O.dct2d_blocks(_blocks(O.rgb_to_ycbcr(f)[..., 0], b)) for f in (cov, emb)])
        U, Vt, S = np.empty_like(D), np.empty_like(D), np.empty((len(D), b), np.float32)
        for reverse in (0, 1):
            for want_v in (1, 0):
                if L.lp_host_svd_blocks(D.ctypes.data, len(D), b, U.ctypes.data if want_v else None, S.ctypes.data,
                                        Vt.ctypes.data if want_v else None, want_v, reverse):
                    raise RuntimeError("the host build did not converge")


def measure_header() -> dict:
    """{"lines": n, "reached": n, "unreached": [source text]} of thatsmyface_amd/csrc/tmfwm_lapack.h
    from a `hipcc --cuda-host-only --coverage -O0` build of tests/native/lp_host.cpp (clang writes
    gcov-compatible notes).  A line counts as reached if any template instantiation reached it."""
    with tempfile.TemporaryDirectory(prefix="lp_coverage_hdr_") as tmp:
        so = os.path.join(tmp, "liblp_host_cov.so")
        subprocess.run([HIPCC if os.path.exists(HIPCC) else "hipcc", "-x", "hip", "--cuda-host-only", "-O0", "--coverage",
                        "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-shared", "-o", so,
                        os.path.join(ROOT, "tests", "native", "lp_host.cpp")], cwd=tmp, check=True, stderr=subprocess.DEVNULL)
        subprocess.run([sys.executable, os.path.abspath(__file__), "--header-child", "--so", so], check=True, cwd=tmp)
        gcda = [f for f in os.listdir(tmp) if f.endswith(".gcda")]
        subprocess.run(["gcov", "-b", "-c", *gcda], cwd=tmp, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        lines: dict = {}
        with open(os.path.join(tmp, HDR + ".gcov")) as f:
            for raw in f:
                m = _LINE.match(raw)
                if not m or m.group(1).strip() == "-":
                    continue
                ln, text = int(m.group(2)), m.group(3).strip()
                hit = m.group(1).strip() not in ("#####", "=====")
                lines[ln] = (text, lines.get(ln, ("", False))[1] or hit)
    # closing braces carry the counter of the jump past an else: not statements of their own
    code = {ln: v for ln, v in lines.items() if v[0].strip("{} ") not in ("", "else")}
    return {"source": "thatsmyface_amd/csrc/" + HDR, "build": "hipcc --cuda-host-only --coverage -O0 tests/native/lp_host.cpp",
            "lines": len(code), "reached": sum(h for _, h in code.values()),
            "unreached": [t for _, (t, h) in sorted(code.items()) if not h]}


def _union(res: dict, corpora) -> dict:
    """routine -> ({lineno: hit}, {branch: taken}) over the given corpora."""
    out: dict = {}
    for c in corpora:
        for fn, d in res[c].items():
            L, B = out.setdefault(fn, ({}, {}))
            for ln, (_, hit) in d["lines"].items():
                L[ln] = L.get(ln, False) or hit
            for key, t in d["branches"].items():
                B[key] = B.get(key, False) or t
    return out


def unreached(res: dict) -> list:
    """[{routine, line}] -- the stripped source text of every line no corpus reached."""
    any_c = next(iter(res.values()))
    out = []
    for fn, (L, _) in sorted(_union(res, res.keys()).items()):
        for ln in sorted(L):
            if not L[ln]:
                out.append({"routine": fn, "line": any_c[fn]["lines"][ln][0]})
    return out


def summary(res: dict) -> dict:
    """Per routine and in total: lines and branch directions, reached by the covers, by covers +
    patterns (everything an embed or extract call reaches), and by all corpora; and the source
    lines that only the stage entry points (matrices, bidiagonals) reach."""
    steps = {"covers": ("covers",), "patterns": ("patterns",), "covers+patterns": ("covers", "patterns"),
             "matrices": ("matrices",), "bidiagonals": ("bidiagonals",), "all": tuple(res.keys())}
    steps = {k: v for k, v in steps.items() if all(c in res for c in v)}
    un = {k: _union(res, v) for k, v in steps.items()}
    routines = sorted(un["all"], key=lambda fn: min(un["all"][fn][0], default=0))
    rows = []
    for fn in routines + ["total"]:
        fns = routines if fn == "total" else [fn]
        row = {"routine": fn, "lines": sum(len(un["all"][f][0]) for f in fns), "branches": sum(len(un["all"][f][1]) for f in fns)}
        for k in steps:
            row["lines_" + k] = sum(sum(un[k].get(f, ({}, {}))[0].values()) for f in fns)
            row["branches_" + k] = sum(sum(un[k].get(f, ({}, {}))[1].values()) for f in fns)
        rows.append(row)
    stage_only = []
    if "covers+patterns" in un:
        any_c = next(iter(res.values()))
        for fn in routines:
            for ln, hit in sorted(un["all"][fn][0].items()):
                if hit and not un["covers+patterns"][fn][0].get(ln, False):
                    stage_only.append({"routine": fn, "line": any_c[fn]["lines"][ln][0]})
    return {"rows": rows, "stage_entry_only_lines": stage_only, "unreached": unreached(res)}


def table(s: dict) -> str:
    cols = [c for c in ("covers", "patterns", "covers+patterns", "matrices", "bidiagonals", "all") if "lines_" + c in s["rows"][0]]
    out = ["| routine | lines | " + " | ".join(cols) + " | branch directions | " + " | ".join(cols) + " |",
           "|---|---|" + "---|" * (2 * len(cols) + 1)]
    for r in s["rows"]:
        out.append("| `%s` | %d | %s | %d | %s |" % (r["routine"], r["lines"], " | ".join(str(r["lines_" + c]) for c in cols),
                                                   r["branches"], " | ".join(str(r["branches_" + c]) for c in cols)))
    return "\n".join(out)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--json", help="write the summary here")
    ap.add_argument("--noise-size", default="1080x1920", help="the covers corpus' noise frame, HxW")
    ap.add_argument("--unreached", action="store_true", help="print the unreached lines")
    ap.add_argument("--no-header", action="store_true", help="skip the device header's own host-build coverage")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    ap.add_argument("--header-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--so", help=argparse.SUPPRESS)
    a = ap.parse_args()
    hw = tuple(int(v) for v in a.noise_size.split("x"))
    if a.child:
        child(a.child, a.so, hw)
        return
    if a.header_child:
        header_child(a.so)
        return
    if not available():
        sys.exit("lp_coverage: needs gcc, g++ and gcov")
    s = summary(measure(hw))
    print(table(s))
    print("\nlines only the stage entry points reach: %d; unreached: %d" % (len(s["stage_entry_only_lines"]), len(s["unreached"])))
    if a.unreached:
        for u in s["unreached"]:
            print("  %-14s %s" % (u["routine"], u["line"]))
    if not a.no_header and header_available():
        s["device_header"] = h = measure_header()
        print("\n%s (host build, all corpora but the covers): %d of %d lines reached" % (h["source"], h["reached"], h["lines"]))
        if a.unreached:
            for t in h["unreached"]:
                print("  " + t)
    else:
        print("\ndevice header: not measured (no hipcc, or --no-header)")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump({"source": "oracle/" + SRC, "build": "gcc --coverage -O0", "noise_size": a.noise_size, **s}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
