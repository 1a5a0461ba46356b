"""Blocks whose rank-1 pre-pass decision is known in advance -- test infrastructure only.

The pre-pass (thatsmyface_amd/csrc/tmfwm_rank1_body.h) keeps a block's bytes when its
gate passes (a zero block, or gap > 0, g1 > 0 and eps_uv <= 2^-30) and every pixel has the same
three bytes at both ends of [Y_fast - eps_Y, Y_fast + eps_Y]; it hands every other block on, and
the routes count those (`lapack_blocks` on rank1_reference, `list_pass_blocks` on rank1).  Blocks
are independent, so a frame built of blocks that all must be refused, or all must be kept, turns
those counts into a statement about the kernel's bound.

The classes come from the one numpy restatement of the bound, tools/exp/fastpath_study.
certify_rank1, evaluated in f64 with eps_Y scaled by k (`decided_k`; monotone in k):
  must-refuse   not decided_0.98
  must-accept   decided_1.02 with the gate tightened to eps_uv <= 2^-31
  unclassified  the rest; no test uses them.
Why a 2 % band is (far) enough.  The kernel evaluates the same expression as the restatement, in
f32 where the restatement uses f64: every factor that enters eps_Y is rounded upward by
(1 + 2^-20), and the sums are a handful of fmaf roundings (2^-24 each, a few tens of them), so the
kernel's eps_Y lies within about 1e-5 relative of the restatement's -- two thousand times inside
the band.  Y_fast is the f32 IDCT (bit exact on both sides) of M_fast = f32(D + c u v^T); the
kernel's f64 power iteration and numpy's einsum round differently, so the two M_fast differ only
where an f64 entry lies within ~1e-15 relative of an f32 rounding midpoint, and then by one f32 ulp
of M, which moves Y_fast by less than eps_Y's own |Y| 2^-22 term.  eps_uv itself agrees to ~1e-13
relative (it is an f64 expression on both sides), so a factor of two on the gate is ample.  The
band is chosen from this reasoning, not measured on the kernel.
"""
from __future__ import annotations

import functools
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
for _p in (_ROOT, _HERE, os.path.join(_ROOT, "tools", "exp")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from oracle import oracle as O  # noqa: E402
import fastpath_study as F  # noqa: E402
from keyed_helpers import sparks  # noqa: E402
from lapack_path import photo_cover  # noqa: E402

SIZES = (4, 6, 8, 10, 12, 14, 16)
REFUSE_SCALE, ACCEPT_SCALE = 0.98, 1.02  # the band
SENTINEL_SCALE, MIRROR_SCALE = 0.90, 1.10  # a bound 10 % too small keeps a sentinel; 10 % too large refuses a mirror
SCALES = (SENTINEL_SCALE, REFUSE_SCALE, 1.0, ACCEPT_SCALE, MIRROR_SCALE)
PHOTO_SEEDS = tuple(range(13, 21))
ALPHAS = (0.1, 1.0, -0.5)


def frame_size(b: int) -> tuple[int, int]:
    return 34 * b, 60 * b


def tiles(b: int, seed: int) -> dict[str, np.ndarray]:
    H, W = frame_size(b)
    tn = O.synth_bytes(0x5EED0002, seed, 1, (H // b) * (W // b)).reshape(H // b, W // b)
    return {"noise": tn, "binary": (tn & 1) * 255}


@functools.lru_cache(maxsize=None)
def pool_frames(b: int):
    """(name, cover, tile, alpha) of every frame of the pool at block size b (shared: read only)."""
    from golden.gen_golden import cover

    H, W = frame_size(b)
    out = []
    for s in PHOTO_SEEDS:
        for wm, t in tiles(b, s).items():
            out.append((f"photo{s}/{wm}", photo_cover(H, W, s), t, 0.1))
    for s in PHOTO_SEEDS[:2]:
        for alpha in ALPHAS[1:]:
            for wm, t in tiles(b, s).items():
                out.append((f"photo{s}/{wm}", photo_cover(H, W, s), t, alpha))
    # the gate's own refusals (no spectral gap), zero blocks, DC-only blocks, noise
    tn = tiles(b, 40)["noise"]
    out.append(("sparks", sparks(H, W, b, 41), tn, 0.1))
    for kind in ("qr", "diagonal", "flat", "black"):
        out.append((kind, cover(kind, H, W, 42), tn, 0.1))
    out.append(("noise", O.synth_bytes(0x5EED0001, 43, 1, H * W * 3).reshape(H, W, 3), tn, 0.1))
    return out


def classify(cov: np.ndarray, tile: np.ndarray, b: int, alpha: float, route_check: bool = False) -> dict:
    """certify_rank1's per-block arrays plus the three classes and the sentinels (bool masks)."""
    r = F.certify_rank1(cov, tile, b, alpha, scale=SCALES, per_block=True, route_check=route_check)
    d = r["decided"]
    r["refuse"] = ~d[REFUSE_SCALE]
    r["accept"] = d[ACCEPT_SCALE] & r["gate_tight"]
    r["unclassified"] = ~r["refuse"] & ~r["accept"]
    r["sentinel"] = r["refuse"] & d[SENTINEL_SCALE]
    r["mirror"] = r["accept"] & ~d[MIRROR_SCALE]
    return r


_CAT = ("zero", "gate", "gate_tight", "refuse", "accept", "unclassified", "sentinel", "mirror", "blocks_rgb", "tile")


@functools.lru_cache(maxsize=None)
def pool(b: int, route_check: bool = False) -> dict:
    """The pool at block size b, classified: per-block arrays over every frame's blocks in order,
    `alpha` and `frame` (index into `names`) per block, `decided_1` (the bound as shipped)."""
    parts, alphas, frame, names = [], [], [], []
    for i, (name, cov, t, alpha) in enumerate(pool_frames(b)):
        r = classify(cov, t, b, alpha, route_check)
        parts.append(r)
        n = len(r["tile"])
        alphas.append(np.full(n, alpha))
        frame.append(np.full(n, i))
        names.append(f"{name}/a{alpha}")
    out = {k: np.concatenate([p[k] for p in parts]) for k in _CAT + (("differs",) if route_check else ())}
    out["decided_1"] = np.concatenate([p["decided"][1.0] for p in parts])
    out["alpha"], out["frame"], out["names"] = np.concatenate(alphas), np.concatenate(frame), names
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def classes(b: int, route_check: bool = False) -> dict[str, np.ndarray]:
    """Index sets into pool(b, route_check): must-refuse, must-accept, unclassified."""
    p = pool(b, route_check)
    return {k: np.nonzero(p[k])[0] for k in ("refuse", "accept", "unclassified")}


def retile(blocks_rgb: np.ndarray, tile_bytes: np.ndarray, cols: int):
    """n blocks (n, b, b, 3) with their tile bytes (n,) as an (rows*b, cols*b, 3) frame and its
    (rows, cols) tile, block i at grid position (i // cols, i % cols); the last row is filled by
    repeating the members from the first on (so the frame holds blocks of the one class only)."""
    n, b = blocks_rgb.shape[:2]
    assert n > 0 and tile_bytes.shape == (n,)
    rows = -(-n // cols)
    idx = np.arange(rows * cols) % n
    fr = blocks_rgb[idx].reshape(rows, cols, b, b, 3).transpose(0, 2, 1, 3, 4).reshape(rows * b, cols * b, 3)
    return np.ascontiguousarray(fr), np.ascontiguousarray(tile_bytes[idx].reshape(rows, cols))
