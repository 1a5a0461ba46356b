"""The embed kernels' key decision (thatsmyface_amd/csrc/tmfwm_embed_key.h) restated
in numpy from the oracle's Jacobi route -- test infrastructure only.  For every block: is it
certified (not zero, not flat, not flagged), and do the two pre-blend ends of sigma_1,
[f32(max(sigma_1 - tE, 0)), f32(sigma_1 + tE)] with tE = 2^-45 sigma_1 for a certified block and 0
otherwise, round to one float (decided) or to two (the block goes to the dgesdd route)."""
from __future__ import annotations

import numpy as np

from oracle import oracle as O

CERT_SCALE = 2.0 ** -45  # tmfwm_blocks.h kCertScale


def blocks_of(rgb: np.ndarray, b: int) -> np.ndarray:
    """The (nbh * nbw, b, b) f32 DCT blocks of a frame's luma, row-major over the block grid."""
    rgb = np.ascontiguousarray(rgb, np.uint8)
    H, W = rgb.shape[:2]
    nbh, nbw = H // b, W // b
    y = O.rgb_to_ycbcr(rgb)[..., 0]
    blocks = np.ascontiguousarray(y[: nbh * b, : nbw * b].reshape(nbh, b, nbw, b).transpose(0, 2, 1, 3).reshape(-1, b, b))
    return O.dct2d_blocks(blocks)


def decide(sigma: np.ndarray, tE: np.ndarray):
    """(decided, key) of f64 sigma_1 and tE, elementwise: embed_key_of in numpy."""
    sigma, tE = np.asarray(sigma, np.float64), np.asarray(tE, np.float64)
    lo = np.maximum(sigma - tE, 0.0).astype(np.float32)
    hi = (sigma + tE).astype(np.float32)
    return (lo.view(np.uint32) == hi.view(np.uint32)) & np.isfinite(lo), lo


def predict_blocks(D: np.ndarray):
    """(certified, decided, key) per block of (n, b, b) f32 DCT blocks: the strip pass's view."""
    D = np.ascontiguousarray(D, np.float32)
    n, b = D.shape[0], D.shape[-1]
    sig = O.svd_blocks_f64(D)[1]  # sorted, descending
    s1 = sig[:, 0]
    # the conditioning test (tmfwm_blocks.h): m = min over triplets reaching the output of
    # min(sigma_k, distance to the nearest other sigma); flagged iff m * 2^20 < sigma_1
    d = np.abs(sig[:, :, None] - sig[:, None, :])
    d[:, np.arange(b), np.arange(b)] = np.inf
    g = np.minimum(sig, d.min(axis=2))
    out = sig.astype(np.float32) != 0.0
    m = np.where(out, g, np.inf).min(axis=1)
    m = np.minimum(m, s1)
    flagged = m * 1048576.0 < s1
    flat = ~(D.reshape(n, -1)[:, 1:] != 0.0).any(axis=1)
    cert = (s1 != 0.0) & ~flat & ~flagged
    decided, key = decide(s1, np.where(cert, CERT_SCALE * s1, 0.0))
    return cert, decided, key


def predict(rgb: np.ndarray, b: int):
    """predict_blocks over a frame: three (H//b, W//b) arrays."""
    H, W = rgb.shape[:2]
    return tuple(a.reshape(H // b, W // b) for a in predict_blocks(blocks_of(rgb, b)))
