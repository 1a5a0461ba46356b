"""CPU side of the rank-1 pre-pass's decision tests: the conditions that
tests/test_rank1_decisions_gpu.py leans on -- none of them a measurement of the kernel -- and the
two measured LAPACK constants held to one value everywhere they are written down.

The classes (tests/rank1_classes.py) come from the one numpy restatement of the bound,
tools/exp/fastpath_study.certify_rank1; the band (0.98 / 1.02) is derived there, not measured."""
import glob
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tools", "exp"), os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import rank1_classes as RC  # noqa: E402


@pytest.mark.parametrize("b", RC.SIZES)
def test_pool_classes(b):
    """The pool classifies almost every block, both classes and both kinds of sentinel are well
    populated, the gate alone refuses hundreds of blocks and zero blocks are among the kept; and
    the restatement is sound on this pool: every block decided at scale 1.0 has the dgesdd route's
    bytes (np.linalg.svd's arithmetic), the engineered covers included."""
    p = RC.pool(b, True)
    n = len(p["tile"])
    count = {k: int(p[k].sum()) for k in ("refuse", "accept", "unclassified", "sentinel", "mirror")}
    assert count["refuse"] + count["accept"] + count["unclassified"] == n and not (p["refuse"] & p["accept"]).any()
    assert n >= 2 * len(RC.PHOTO_SEEDS) * 2040
    assert count["unclassified"] <= 0.02 * n, count
    assert count["refuse"] >= 1000 and count["accept"] >= 1000, count
    assert int((p["refuse"] & ~p["gate"]).sum()) >= 300, count
    assert int((p["accept"] & p["zero"]).sum()) >= 100, count
    assert count["sentinel"] >= 30 and count["mirror"] >= 30, count
    # every alpha group can fill its own frames of each class, sentinels included
    for alpha in RC.ALPHAS:
        m = p["alpha"] == alpha
        assert min(int((p[k] & m).sum()) for k in ("refuse", "accept", "sentinel", "mirror")) >= 30, (alpha, count)
    # decided_k is monotone in k: the sentinels are decided at 0.90 and not at 0.98, and a decided
    # block passed the gate
    assert not (p["decided_1"] & ~p["gate"]).any() and not (p["accept"] & ~p["decided_1"]).any()
    assert not (p["refuse"] & p["decided_1"]).any()
    assert int((p["decided_1"] & p["differs"]).sum()) == 0
    assert int(p["decided_1"].sum()) > n // 4  # the soundness check is not vacuous


@pytest.mark.parametrize("b", [4, 10, 16])
@pytest.mark.parametrize("cols", [64, 35])
def test_retiling_keeps_the_class(b, cols):
    """Blocks are independent: a class re-tiled into a frame of its own (full and partial last
    row) classifies as that class again, block for block, and retile puts block i at (i // cols,
    i % cols) with its own tile byte."""
    p = RC.pool(b, True)
    m = p["alpha"] == 1.0
    for k in ("refuse", "accept"):
        idx = np.nonzero(p[k] & m)[0][:700]
        fr, t = RC.retile(p["blocks_rgb"][idx], p["tile"][idx], cols)
        rows = -(-len(idx) // cols)
        assert fr.shape == (rows * b, cols * b, 3) and t.shape == (rows, cols)
        i = len(idx) - 1
        assert np.array_equal(fr[(i // cols) * b:(i // cols + 1) * b, (i % cols) * b:(i % cols + 1) * b], p["blocks_rgb"][idx[i]])
        assert t[i // cols, i % cols] == p["tile"][idx[i]]
        r = RC.classify(fr, t, b, 1.0)
        assert r[k].all(), (k, int(r[k].sum()), rows * cols)
        for name in ("gate", "zero", "sentinel", "mirror"):
            assert np.array_equal(r[name][: len(idx)], p[name][idx]), (k, name)


def test_restatement_carries_the_kernels_gate():
    """certify_rank1's default result refuses what the kernel's eps_uv <= 2^-30 gate refuses: a
    frame's undecided fraction is the per-block decision's at scale 1 up to the two tails'
    different slack, and `scale` moves it monotonically."""
    import fastpath_study as F

    b = 8
    name, cov, t, alpha = RC.pool_frames(b)[0]
    und = [F.certify_rank1(cov, t, b, alpha, scale=k, route_check=False)["undecided"] for k in (0.5, 1.0, 2.0)]
    assert und[0] < und[1] < und[2], und
    r = RC.classify(cov, t, b, alpha)
    assert abs(und[1] - (1 - r["decided"][1.0].mean())) < 0.02, und
    assert F.GATE_EPS_UV == 2.0 ** -30
    assert np.array_equal(r["gate"], r["zero"] | (r["gate"] & (r["eps_uv"] <= F.GATE_EPS_UV)))
    assert not (r["gate_tight"] & ~r["gate"]).any()


def test_lapack_constants_agree_and_keep_their_margins():
    """The two measured LAPACK constants of the pre-pass (residual: 8192 units of 2^-53 s1 = 2^-40
    s1; top pair: 1024 units) are one value in the kernel's source, tests/k_corpus.py, the numpy
    restatement, tools/exp/lapack_bounds.py and every measured profile, and the measured maxima
    stay at least 80x (residual) and 6x (top pair) below them."""
    import fastpath_study as F
    import k_corpus as kc
    import lapack_bounds as LB

    # the pre-pass's whole source: the constants' home, the one body, and its two kernels
    src = ""
    for name in ("tmfwm_rank1.h", "tmfwm_rank1_body.h", "tmfwm_rank1.hip", "tmfwm_ragged_pre.hip"):
        with open(os.path.join(ROOT, "thatsmyface_amd", "csrc", name)) as f:
            src += f.read() + "\n"
    defs = re.findall(r"constexpr double (kRank1\w+Units) = ([0-9.]+);", src)
    named = sorted((n, float(v)) for n, v in defs)  # a list: a second definition anywhere fails
    assert named == [("kRank1PairUnits", float(kc.PAIR_UNITS)), ("kRank1ResidUnits", float(kc.RESID_UNITS))], named
    # the names are what the kernels use: over the four files each occurs twice, one definition
    # and one use (the body is one text), and the bare literals are gone (comments aside)
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert code.count("kRank1ResidUnits") == 2 and code.count("kRank1PairUnits") == 2
    assert "0x1p-40f * s1f" not in code and "1024.0 * u53" not in code
    assert kc.RESID_UNITS * 2.0 ** -53 == 2.0 ** -40
    assert (F.RESID_UNITS, F.PAIR_UNITS) == (kc.RESID_UNITS, kc.PAIR_UNITS) == (LB.RESID_UNITS, LB.PAIR_UNITS)
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r06", "lapack_bounds_b*.json")))
    assert {os.path.basename(p) for p in files} == {f"lapack_bounds_b{b}.json" for b in RC.SIZES}
    for path in files:
        with open(path) as f:
            r = json.load(f)
        assert r["resid_bound_units"] == kc.RESID_UNITS and r["pair_bound_units"] == kc.PAIR_UNITS, path
        assert r["resid_max"] > 0 and r["resid_max"] * 80 <= kc.RESID_UNITS, (path, r["resid_max"])
        assert r["top_pair_max"] > 0 and r["top_pair_max"] * 6 <= kc.PAIR_UNITS, (path, r["top_pair_max"])
