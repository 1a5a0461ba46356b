"""Expected values of keyed extraction from the oracle's stages -- test
infrastructure only.  A key entry is the dgesdd route's f32 S[0] of a block's DCT; the byte is
the reference's watermarking.py:285-289 on two such floats."""
from __future__ import annotations

import numpy as np

from oracle import oracle as O


def key_of(rgb: np.ndarray, b: int) -> np.ndarray:
    """f32 (H//b, W//b): np.linalg.svd's f32 S[0] of every block's DCT (the oracle's dgesdd route)."""
    rgb = np.ascontiguousarray(rgb, np.uint8)
    H, W = rgb.shape[:2]
    nbh, nbw = H // b, W // b
    y = O.rgb_to_ycbcr(rgb)[..., 0]
    blocks = np.ascontiguousarray(y[: nbh * b, : nbw * b].reshape(nbh, b, nbw, b).transpose(0, 2, 1, 3).reshape(-1, b, b))
    return np.ascontiguousarray(O.lp_svd_blocks(O.dct2d_blocks(blocks))[1][:, 0].reshape(nbh, nbw))


def bytes_of(kw: np.ndarray, ko: np.ndarray, alpha: float) -> np.ndarray:
    """trunc(clip(f64((k_w - k_o) / f32(alpha)), 0, 1) * 255) for finite keys."""
    with np.errstate(over="ignore"):
        e = (kw.astype(np.float32) - ko.astype(np.float32)) / np.float32(alpha)
    return (np.clip(e.astype(np.float64), 0.0, 1.0) * 255.0).astype(np.uint8)


def sparks(H: int, W: int, b: int, seed: int) -> np.ndarray:
    """A black frame whose every b x b block holds a random permutation matrix of white pixels:
    all singular values of such a block's DCT are equal, so 2 sigma_1^2 <= |D|_F^2 and the
    sigma_1 enclosure (which needs 2 rho > F) can never decide -- every block takes the dgesdd
    route.  Pixels outside the block grid stay black."""
    rng = np.random.default_rng(seed)
    img = np.zeros((H, W, 3), np.uint8)
    for bi in range(H // b):
        for bj in range(W // b):
            p = rng.permutation(b)
            img[bi * b + np.arange(b), bj * b + p] = 255
    return img
