"""Certified rank-1 embed ("fast path", SURVEY 7 H2 / VERDICT r03 item 4): how many blocks can
skip the full SVD with a rigorous proof that their output bytes are the reference's?

The reference (watermarking.py:192-216) computes per block M_ref = fl(U32 @ fl(S'32 * Vt32))
from LAPACK's factors rounded to f32, then Y_ref = IDCT_fl(M_ref) and the bytes.  Because only
S[0] changes, M_ref = D + c u1 v1^T + (rounding terms), c = alpha * w / 255.  The fast path
computes M_fast = f32(D + c u1 v1^T) from the top singular pair alone, Y_fast = IDCT_fl(M_fast),
and a per-pixel bound eps_Y >= |Y_ref - Y_fast|:

  dM_ij <= 1.01 [(b+5) u (G_ij + c P_ij) + 2u (s1 + c) P_ij] + eps_A + 2 c eps_uv
    u = 2^-24; G_ij = sqrt(|D_i,:| |D_:,j|) bounds sum_t |U_it| s_t |V_jt| (Cauchy-Schwarz twice,
    rows of U and V are unit vectors); P_ij = |u1_i| |v1_j|; eps_A = K_A 2^-53 s1 (LAPACK's
    residual |U S V^T - D|, K_A = 1024); eps_uv bounds the top pair's disagreement (K 2^-53 s1/gap1);
    the (b+5) u counts the b fmaf roundings of the chain, 4 factor roundings and the f32(M_fast);
  eps_Y = kappa |C| (dM + 2 gamma_L (|M_fast| + dM)) |C|^T   (linear part + both IDCT roundings;
    |C| the exact ortho DCT-III matrix, kappa = 2, L = 16 as the pocketfft depth allowance) --
    round 4's allowance, kept here as that study ran; the shipped pre-pass and certify_rank1 below
    use the IDCT rounding bound derived from the op sequence (tools/exp/idct_bound.py), which this
    allowance undercuts where |C| is small.
A channel byte is certain when the colour inverse (monotone in Y, slope 1) gives the same byte
for every Y in [Y_fast - eps_Y, Y_fast + eps_Y] (f32 rounding slack included); a block is
certified when all its bytes are.  Reported: certified fraction, and that every certified
block's bytes equal the dgesdd route's (np.linalg.svd's arithmetic).
usage: fastpath_study.py B FRAMES_PER_KIND [H W]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import oracle as O  # noqa: E402
import idct_bound as IB  # noqa: E402
from lapack_path import _blocks, _unblocks, photo_cover  # noqa: E402
from cert_study import lp_f64  # noqa: E402

import k_corpus as KC  # noqa: E402

U32 = 2.0**-24
EPS = 2.0**-53
# LAPACK's two measured constants of the rank-1 pre-pass, in units of 2^-53 s1 (the kernel's
# kRank1ResidUnits / kRank1PairUnits, csrc/tmfwm_rank1.h; tools/exp/lapack_bounds.py measures them)
RESID_UNITS = KC.RESID_UNITS
PAIR_UNITS = KC.PAIR_UNITS
GATE_EPS_UV = 2.0**-30  # the pre-pass refuses a block whose top pair is known no better than this


def dct_matrix(b):
    """exact orthonormal DCT-II matrix C (Y = C X C^T); its transpose is the DCT-III."""
    k = np.arange(b)[:, None]
    n = np.arange(b)[None, :]
    C = np.cos(np.pi * (2 * n + 1) * k / (2 * b)) * np.sqrt(2.0 / b)
    C[0] /= np.sqrt(2.0)
    return C


def byte_of(t):
    """u8_from_unit of an f64 colour value already rounded to f32"""
    return np.floor(np.clip(t.astype(np.float32), 0, 1) * np.float32(255)).astype(np.int64)


def certify(cov, tile, b, alpha=0.1, K_A=1024.0, K_uv=1024.0, kappa=2.0, L=16, route_check=True):
    H, W = cov.shape[:2]
    nbh, nbw = H // b, W // b
    ycc = O.rgb_to_ycbcr(cov)
    D = O.dct2d_blocks(_blocks(ycc[..., 0], b))
    Ul, sl, Vtl = lp_f64(D)
    n = len(D)
    s1 = sl[:, 0]
    u1 = Ul[:, :, 0]
    v1 = Vtl[:, 0, :]
    c = alpha * (tile.reshape(-1).astype(np.float64) / 255.0)
    D64 = D.astype(np.float64)
    Mf = (D64 + c[:, None, None] * u1[:, :, None] * v1[:, None, :]).astype(np.float32)
    Yf = O.dct2d_blocks(Mf, inverse=True)
    # bound
    r = np.sqrt((D64**2).sum(axis=2)) * (1 + 1e-12)
    cn = np.sqrt((D64**2).sum(axis=1)) * (1 + 1e-12)
    G = np.sqrt(r[:, :, None] * cn[:, None, :])
    P = np.abs(u1)[:, :, None] * np.abs(v1)[:, None, :]
    F = (D64**2).sum(axis=(1, 2))
    s2 = np.sqrt(np.maximum(F - s1**2, 0))
    gap = np.maximum(s1 - s2, 1e-300)
    eps_uv = K_uv * EPS * s1 / gap
    dM = 1.01 * ((b + 5) * U32 * (G + c[:, None, None] * P) + 2 * U32 * (s1 + c)[:, None, None] * P) \
        + (K_A * EPS * s1)[:, None, None] + (2 * c * eps_uv)[:, None, None]
    gL = L * U32 / (1 - L * U32)
    X = dM + 2 * gL * (np.abs(Mf.astype(np.float64)) + dM)
    C = np.abs(dct_matrix(b))
    epsY = kappa * np.einsum("ai,nij,bj->nab", C.T, X, C.T)  # DCT-III = C^T
    # per pixel / channel certainty
    Yp = _unblocks(Yf, nbh, nbw, b).astype(np.float64)
    Ep = _unblocks(epsY, nbh, nbw, b)
    cbp = (ycc[: nbh * b, : nbw * b, 1] - np.float32(0.5)).astype(np.float64)
    crp = (ycc[: nbh * b, : nbw * b, 2] - np.float32(0.5)).astype(np.float64)
    ok = np.ones(Yp.shape, bool)
    for a_cr, a_cb in ((1.403, 0.0), (-0.714, -0.344), (0.0, 1.773)):
        base = a_cr * crp + a_cb * cbp
        t = Yp + base
        slack = Ep * (1 + 1e-9) + 2 * U32 * np.abs(t) + 1e-12
        lo, hi = t - slack, t + slack
        plo = np.where(lo >= 1, 255.0, np.clip(lo, 0, 1) * 255.0 * (1 - 2**-21) - 1e-9)
        phi = np.where(hi <= 0, 0.0, np.clip(hi, 0, 1) * 255.0 * (1 + 2**-21) + 1e-9)
        ok &= (np.floor(np.maximum(plo, 0)) == np.floor(np.minimum(phi, 255.0)))
    cert = ok.reshape(nbh, b, nbw, b).all(axis=(1, 3)).reshape(-1)
    res = {"blocks": n, "certified": int(cert.sum()), "frac_exact_path": 1 - float(cert.mean()),
           "epsY_median_bytes": float(np.median(epsY) * 255)}
    if route_check:
        # certified blocks' bytes must be the dgesdd route's
        out_fast = ycc.copy()
        out_fast[: nbh * b, : nbw * b, 0] = _unblocks(Yf, nbh, nbw, b)
        fast = O.ycbcr_to_rgb(out_fast)
        ref = O.embed_frame(cov, tile, b, alpha, route="lapack")
        bd = (fast != ref)[: nbh * b, : nbw * b].reshape(nbh, b, nbw, b, 3).any(axis=(1, 3, 4)).reshape(-1)
        res["certified_blocks_differing_from_lapack"] = int((bd & cert).sum())
        res["uncertified_blocks_differing"] = int((bd & ~cert).sum())
    return res


def certify_rank1(cov, tile, b, alpha=0.1, iters=4, scale=1.0, per_block=False, route_check=True):
    """The shipped pre-pass's bound (csrc/tmfwm_rank1.h, tmfwm_rank1_body.h, round 6) restated in numpy: the top
    pair from `iters` f64 power steps on D^T D from the column-norm vector with the a-posteriori
    angle (Kato-Temple margins, Davis-Kahan) plus LAPACK's 1024 2^-53 s1 / (s1 - s2); dM in rank-one
    form (alpha' G + beta' P + gamma'); the IDCT roundings through |M_fast| <= G + |c| P; bytes at
    both ends of [Y_fast - eps_Y, Y_fast + eps_Y].  The gate is the kernel's: a zero block, or
    gap > 0, g1 > 0 and eps_uv <= 2^-30.  `scale` multiplies eps_Y (1.0: the bound as shipped).
    Returns the undecided fraction and the number of decided blocks whose bytes differ from the
    dgesdd route's (the soundness check).

    per_block=True returns per-block arrays in block order (row-major over the block grid) instead:
    `scale` may then be a sequence, and `decided[k]` for a scale k is the kernel's own rule with
    eps_Y scaled -- the gate passes and the exact colour tail (O.ycbcr_to_rgb on the frame's own
    chroma, the device's f32-plus-f64-redo tail equals it) gives the same three bytes at
    f32(Y_fast - k eps_Y) and f32(Y_fast + k eps_Y) for every pixel.  Bytes are monotone in Y, so
    decided[k] is monotone in k.  Also: `zero`, `gate`, `gate_tight` (eps_uv <= 2^-31: a block this
    far inside the gate passes the kernel's whatever its f64 roundings), `eps_uv`, the cover's
    blocks `blocks_rgb` (n, b, b, 3), their `tile` bytes (n,), and with route_check `differs`: the
    blocks whose fast bytes are not the dgesdd route's."""
    H, W = cov.shape[:2]
    nbh, nbw = H // b, W // b
    ycc = O.rgb_to_ycbcr(cov)
    D = O.dct2d_blocks(_blocks(ycc[..., 0], b))
    D64 = D.astype(np.float64)
    n = len(D)
    rn = (D64**2).sum(axis=2)
    cn = (D64**2).sum(axis=1)
    F = cn.sum(axis=1)
    zero = F == 0
    v = np.where(zero[:, None], np.eye(b)[0][None, :], cn)
    for _ in range(iters):
        w = np.einsum("nij,ni->nj", D64, np.einsum("nij,nj->ni", D64, v))
        nn = (w**2).sum(axis=1)
        live = (nn > 0)[:, None]
        v = np.where(live, w / np.sqrt(np.where(live[:, 0], nn, 1.0))[:, None], v)
    nv = (v**2).sum(axis=1)
    t = np.einsum("nij,nj->ni", D64, v)
    tt = (t**2).sum(axis=1)
    rho = tt / np.where(nv > 0, nv, 1)
    r = np.einsum("nij,ni->nj", D64, t) - rho[:, None] * v
    rr0 = np.sqrt((r**2).sum(axis=1) / np.where(nv > 0, nv, 1)) * (1 + 16 * EPS) + 256 * EPS * F
    rlo, fhi = rho * (1 - 256 * EPS), F * (1 + 256 * EPS)
    gap = 2 * rlo - fhi
    lhi = (rho + rr0**2 / np.where(gap > 0, gap, 1)) * (1 + 256 * EPS)
    s1hi = np.sqrt(lhi) * (1 + 512 * EPS)
    s2hi = np.sqrt(np.maximum(fhi - rlo, 0)) * (1 + 512 * EPS)
    g1 = np.sqrt(rlo) * (1 - 512 * EPS) - s2hi
    e = np.where(zero, 0.0, 1.01 * rr0 / np.where(gap > 0, gap, 1) + PAIR_UNITS * EPS * s1hi / np.where(g1 > 0, g1, 1) + 2.0**-45)
    spectral = (gap > 0) & (g1 > 0)
    ok = zero | (spectral & (e <= GATE_EPS_UV))
    u = np.where(zero[:, None], np.eye(b)[0][None, :], t / np.sqrt(np.where(tt > 0, tt, 1))[:, None])
    v = v / np.sqrt(np.where(nv > 0, nv, 1))[:, None]
    c = alpha * (tile.reshape(-1).astype(np.float64) / 255.0)
    Mf = (D64 + c[:, None, None] * u[:, :, None] * v[:, None, :]).astype(np.float32)
    Yf = O.dct2d_blocks(Mf, inverse=True)
    ca = np.abs(c)
    al = 1.01 * (b + 6) * U32
    be = 1.01 * ((b + 6) * U32 * ca + 2 * U32 * (s1hi + ca))
    ga = RESID_UNITS * EPS * s1hi + ca * e * (2 + e)
    # |M_ref - M_fast| <= dM = al a b^T + be u' v'^T + ga 1 1^T, and both |M_ref|, |M_fast| <= Mb =
    # (1 + al) a b^T + (|c| + be) u' v'^T + ga 1 1^T; through the f32 IDCT (tools/exp/idct_bound.py:
    # IDCT_fl(M) = C' M C'^T + R, |R| <= u (E |M| |C'|^T + |C'| |M| E^T) + u^2 E |M| E^T):
    # eps_Y = |C'| dM |C'|^T + 2 (u (E Mb |C'|^T + |C'| Mb E^T) + u^2 E Mb E^T), every term rank one
    absc, err = (np.array(t) for t in IB.tables(b))  # [p][i]
    a_ = np.sqrt(np.sqrt(rn))
    b_ = np.sqrt(np.sqrt(cn))
    up, vp = np.abs(u) + e[:, None], np.abs(v) + e[:, None]
    one = np.ones((n, b))
    epsY = np.zeros((n, b, b))
    for x_, y_, d_, m_ in ((a_, b_, np.full(n, al), np.full(n, 1 + al)), (up, vp, be, ca + be), (one, one, ga, ga)):
        A, EA = x_ @ absc.T, x_ @ err.T
        Bq, EB = y_ @ absc.T, y_ @ err.T
        epsY += d_[:, None, None] * A[:, :, None] * Bq[:, None, :]
        epsY += (2 * U32 * m_)[:, None, None] * (EA[:, :, None] * Bq[:, None, :] + A[:, :, None] * EB[:, None, :]
                                                 + U32 * EA[:, :, None] * EB[:, None, :])
    epsY = epsY * (1 + 2.0**-16) + np.abs(Yf) * 2.0**-22 + 2.0**-40
    Yp = _unblocks(Yf, nbh, nbw, b).astype(np.float64)
    Ep = _unblocks(epsY, nbh, nbw, b)
    cbp = (ycc[: nbh * b, : nbw * b, 1] - np.float32(0.5)).astype(np.float64)
    crp = (ycc[: nbh * b, : nbw * b, 2] - np.float32(0.5)).astype(np.float64)

    def per_block_any(px):  # (H', W', ...) bool per pixel -> per block
        return px.reshape(nbh, b, nbw, b, -1).any(axis=(1, 3, 4)).reshape(-1)

    def fast_bytes(Y):  # the exact colour tail on the cover's own chroma with the grid's Y replaced
        out = ycc.copy()
        out[: nbh * b, : nbw * b, 0] = Y
        return O.ycbcr_to_rgb(out)[: nbh * b, : nbw * b]

    bd = None
    if route_check:
        ref = O.embed_frame(cov, tile, b, alpha, route="lapack")
        bd = per_block_any(fast_bytes(_unblocks(Yf, nbh, nbw, b)) != ref[: nbh * b, : nbw * b])
    if per_block:
        decided = {}
        for k in np.atleast_1d(scale):
            lo, hi = (Yp - float(k) * Ep).astype(np.float32), (Yp + float(k) * Ep).astype(np.float32)
            decided[float(k)] = ok & ~per_block_any(fast_bytes(lo) != fast_bytes(hi))
        rgb = np.ascontiguousarray(cov[: nbh * b, : nbw * b].reshape(nbh, b, nbw, b, 3).transpose(0, 2, 1, 3, 4).reshape(n, b, b, 3))
        res = {"zero": zero, "gate": ok, "gate_tight": zero | (spectral & (e <= GATE_EPS_UV / 2)), "eps_uv": e,
               "decided": decided, "blocks_rgb": rgb, "tile": np.ascontiguousarray(tile, np.uint8).reshape(-1).copy()}
        if route_check:
            res["differs"] = bd
        return res
    Ep = float(scale) * Ep
    okp = np.ones(Yp.shape, bool)
    for a_cr, a_cb in ((1.403, 0.0), (-0.714, -0.344), (0.0, 1.773)):
        tcol = Yp + a_cr * crp + a_cb * cbp
        slack = Ep + 2 * U32 * np.abs(tcol) + 1e-12
        okp &= byte_of(tcol - slack) == byte_of(tcol + slack)
    cert = okp.reshape(nbh, b, nbw, b).all(axis=(1, 3)).reshape(-1) & ok
    res = {"blocks": n, "undecided": float(1 - cert.mean())}
    if route_check:
        res["decided_blocks_differing"] = int((bd & cert).sum())
    return res


def main():
    b, nfr = int(sys.argv[1]), int(sys.argv[2])
    H, W = (int(x) for x in sys.argv[3:5]) if len(sys.argv) > 4 else (2160, 3840)
    for kind in ("noise", "photo"):
        for f in range(nfr):
            t0 = time.time()
            cov = O.synth_bytes(0x5EED0001, f, 1, H * W * 3).reshape(H, W, 3) if kind == "noise" else photo_cover(H, W, 100 + f)
            tile = O.synth_bytes(0x5EED0002, f, 1, (H // b) * (W // b)).reshape(H // b, W // b)
            print(kind, f, f"{time.time() - t0:.1f}s", certify(cov, tile, b), flush=True)


if __name__ == "__main__":
    main()
