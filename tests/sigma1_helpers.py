"""The extract path's sigma_1 enclosure (sigma1_certified in thatsmyface_amd/csrc/tmfwm_device.h,
DESIGN.md 5) restated in numpy, and the block classes that follow from its margins -- test
infrastructure only.

The kernel decides f32(sigma_1) of a block only when both ends of a Kato-Temple enclosure
[slo, shi] round to one float.  Its f64 margins (256 u on rho and F, 512 u on the square roots,
u = 2^-53) make the enclosure contain sigma_1 (1 -+ 640 u) for ANY power vector, so whether a block
can be decided depends on how far its sigma_1 lies from the nearest midpoint between two floats:

  must refuse  closer than REFUSE units (of 2^-53 sigma_1): the midpoint is inside every enclosure
               the kernel can build, no pass may decide the block;
  must keep    between REFUSE and KEEP_MAX units, and an enclosure twice as wide as this model's
               after the list pass's 8 iterations still decides: the list pass must decide it;
  fill         at least 2^-36 sigma_1 away, and that widened enclosure decides.

LAPACK's sigma_1 is np.linalg.svd's f64 S[0] of the f32 block, the value whose f32 rounding
oracle.lp_svd_blocks returns."""
from __future__ import annotations

import numpy as np

from keyed_helpers import bytes_of
from oracle import oracle as O

U = 2.0 ** -53
REFUSE = 600.0  # 640 u of margin less 40 u for the roundings the margins cover (LAPACK's included)
HALF_WIDTH = 640.0  # 512 u on the square root + half of 256 u under it
KEEP_MAX = 32 * HALF_WIDTH
KEEP_WIDEN = 2.0
FILL_MIN = 2.0 ** 17  # 2^-36 relative
LIST_ITERS = 8  # kListPowerIters
NONE, MUST_REFUSE, MUST_KEEP, FILL = 0, 1, 2, 3


def strip_iters(b: int) -> int:
    """Power steps of the strip pass (kPowerIters = 3; at b = 4 one product with (D^T D)^4)."""
    return 4 if b == 4 else 3


def power_vector(D: np.ndarray, iters: int) -> np.ndarray:
    """The f32 power iteration on D^T D from e0, normalised each step, with the kernel's guard
    against a vanished vector.  Not the kernel's operation order bit for bit."""
    D = np.ascontiguousarray(D, np.float32)
    n, b = D.shape[0], D.shape[-1]
    v = np.zeros((n, b), np.float32)
    v[:, 0] = 1.0
    Dt = np.ascontiguousarray(D.transpose(0, 2, 1))
    for _ in range(iters):
        uu = np.matmul(D, v[:, :, None])
        w = np.matmul(Dt, uu)[:, :, 0]
        nn = np.sum(w * w, axis=1, dtype=np.float32)
        live = nn > np.float32(1e-30)
        inv = np.float32(1.0) / np.sqrt(np.where(live, nn, np.float32(1.0)))
        v = np.where(live[:, None], w * inv[:, None], v).astype(np.float32)
    return v


def tail(x: np.ndarray, vd: np.ndarray):
    """sigma1_certified's f64 tail for f64 blocks x (n, b, b) and vectors vd (n, b):
    (slo, shi, ok, rho)."""
    u = U
    F = np.sum(x * x, axis=(1, 2))
    nv = np.sum(vd * vd, axis=1)
    ud = np.matmul(x, vd[:, :, None])[:, :, 0]
    a = np.sum(ud * ud, axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        rho = a / nv
        g = np.matmul(x.transpose(0, 2, 1), ud[:, :, None])[:, :, 0]
        rj = g - rho[:, None] * vd
        rn2 = np.sum(rj * rj, axis=1)
        rr0 = np.sqrt(rn2 / nv) * (1.0 + 16.0 * u) + 256.0 * u * F
        rr = rr0 * rr0
        rlo = rho * (1.0 - 256.0 * u)
        fhi = F * (1.0 + 256.0 * u)
        gap = (rlo + rlo) - fhi
        hi = (rho + rr / np.where(gap > 0.0, gap, 1.0)) * (1.0 + 256.0 * u)
        slo = np.sqrt(rlo) * (1.0 - 512.0 * u)
        shi = np.sqrt(hi) * (1.0 + 512.0 * u)
    return slo, shi, F, gap, rho


def decides(slo, shi, F, gap, rho):
    with np.errstate(invalid="ignore", over="ignore"):
        same = shi.astype(np.float32) == slo.astype(np.float32)
    return (F == 0.0) | ((gap > 0.0) & same & (rho == rho))


def enclosure(D: np.ndarray, iters: int, widen: float = 1.0):
    """(slo, shi, ok) of sigma1_certified for (n, b, b) f32 DCT blocks after `iters` power steps;
    widen scales the interval about its centre before ok is taken."""
    D = np.ascontiguousarray(D, np.float32)
    slo, shi, F, gap, rho = tail(D.astype(np.float64), power_vector(D, iters).astype(np.float64))
    if widen != 1.0:
        c, h = 0.5 * (slo + shi), 0.5 * (shi - slo) * widen
        slo, shi = c - h, c + h
    return slo, shi, decides(slo, shi, F, gap, rho)


def midpoint_distance(s) -> np.ndarray:
    """Relative distance of f64 s > 0 from the nearest midpoint between two neighbouring floats
    of its binade, in units of 2^-53 (exact in f64 up to the final division; inf at s = 0)."""
    s = np.asarray(s, np.float64)
    m, _ = np.frexp(s)  # s = m 2^e, m in [0.5, 1): floats are 2^-24 apart there
    t = m * 2.0 ** 24
    d = np.abs((t - np.floor(t)) - 0.5)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(s > 0.0, d * 2.0 ** 29 / m, np.inf)


def sigma1_lapack(D: np.ndarray) -> np.ndarray:
    """LAPACK's f64 sigma_1 of f32 blocks as the reference gets it (np.linalg.svd, full factors)."""
    return np.linalg.svd(np.ascontiguousarray(D, np.float32).astype(np.float64))[1][:, 0]


def classify(D: np.ndarray):
    """(class, distance in units, model half-width in units) per block of (n, b, b) f32 D."""
    s = sigma1_lapack(D)
    dist = midpoint_distance(s)
    slo, shi, _ = enclosure(D, LIST_ITERS)
    wide = enclosure(D, LIST_ITERS, widen=KEEP_WIDEN)[2]
    cls = np.full(len(dist), NONE, np.int8)
    cls[(dist >= FILL_MIN) & wide] = FILL
    cls[(dist >= REFUSE) & (dist <= KEEP_MAX) & wide] = MUST_KEEP
    cls[dist < REFUSE] = MUST_REFUSE
    with np.errstate(divide="ignore", invalid="ignore"):
        half = 0.5 * (shi - slo) / (s * U)
    return cls, dist, half


def frame_blocks(rgb: np.ndarray, b: int) -> np.ndarray:
    """(nbh * nbw, b, b) f32 DCT blocks of an RGB u8 frame's luma, row-major over the block grid."""
    rgb = np.ascontiguousarray(rgb, np.uint8)
    H, W = rgb.shape[:2]
    nbh, nbw = H // b, W // b
    y = O.rgb_to_ycbcr(rgb)[..., 0]
    blocks = y[: nbh * b, : nbw * b].reshape(nbh, b, nbw, b).transpose(0, 2, 1, 3).reshape(-1, b, b)
    return O.dct2d_blocks(np.ascontiguousarray(blocks))


def classify_frame(rgb: np.ndarray, b: int):
    """classify over a frame's block grid: (class, distance, half-width), each (nbh, nbw)."""
    nbh, nbw = rgb.shape[0] // b, rgb.shape[1] // b
    return tuple(a.reshape(nbh, nbw) for a in classify(frame_blocks(rgb, b)))


def sharpened_key(key_ref: np.ndarray, sigma: np.ndarray, listed: np.ndarray, alpha: float, seed: int = 0):
    """A key against which one wrong ulp of sigma_1 shows in the byte: (key, sharp).

    key_ref is the frame's own f32 sigma_1 map, sigma LAPACK's f64 sigma_1, listed the blocks to
    sharpen.  Every entry starts at key_ref - alpha j / 255 for a random byte j; a listed block's
    entry is a float next to such a value at which the correct float key_ref gives one byte and the
    float on the other side of the block's nearest midpoint gives another.  sharp marks the listed
    blocks for which such an entry was found."""
    rng = np.random.default_rng(seed)
    a64 = float(np.float32(alpha))
    key = (key_ref.astype(np.float64) - a64 * rng.integers(1, 255, key_ref.shape) / 255.0).astype(np.float32)
    sharp = np.zeros(key_ref.shape, bool)
    off = np.arange(-8, 9)
    for pos in map(tuple, np.argwhere(listed)):
        sw = key_ref[pos]
        other = np.nextafter(sw, np.float32(np.inf if sigma[pos] > float(sw) else -np.inf))
        for j in rng.permutation(np.arange(1, 255)):  # the few floats around sw - alpha j / 255, one byte edge after another
            c = np.float32(float(sw) - a64 * j / 255.0)
            if not c > 0.0:  # positive floats: neighbours are neighbouring bit patterns
                continue
            cand = (c.view(np.uint32).astype(np.int64) + off).astype(np.uint32).view(np.float32)
            hit = np.flatnonzero(bytes_of(np.full(len(cand), sw), cand, alpha) != bytes_of(np.full(len(cand), other), cand, alpha))
            if len(hit):
                key[pos] = cand[hit[np.argmin(np.abs(off[hit]))]]
                sharp[pos] = True
                break
    return key, sharp


BYTE_ALPHAS = (0.01, 0.05, 0.1, 0.15, 0.2, 0.3, 1.0, -0.5)


def byte_edge_points(alpha: float) -> np.ndarray:
    """f32 numerators d at which extract_byte's (d / f32(alpha)) changes the byte or meets an
    edge: the 7 floats around f32(f64(alpha32) k / 255) for k = 1..255, +-0, the smallest
    subnormal, alpha32 and its two neighbours (bytes 254 / 255), 1e38 and 3e38 (for |alpha| < 1 the
    quotient overflows to infinity), and the negatives of the last three groups (byte 0)."""
    a32 = np.float32(alpha)
    sign = np.float32(np.sign(a32))
    c = np.abs((np.float64(a32) * np.arange(1, 256) / 255.0).astype(np.float32))
    around = (c.view(np.uint32).astype(np.int64)[:, None] + np.arange(-3, 4)[None, :]).astype(np.uint32).view(np.float32).ravel()
    tiny = np.float32(1e-45)
    am = np.abs(a32)
    edges = np.float32([tiny, np.nextafter(am, np.float32(0)), am, np.nextafter(am, np.float32(np.inf)), 1e38, 3e38])
    return np.concatenate([sign * around, np.float32([0.0, -0.0]), sign * edges, -sign * edges]).astype(np.float32)


def byte_by_reciprocal(d: np.ndarray, alpha: float) -> np.ndarray:
    """The byte of a kernel that multiplied by 1 / alpha32 instead of dividing (what the sweep must show)."""
    with np.errstate(over="ignore"):
        e = np.asarray(d, np.float32) * (np.float32(1.0) / np.float32(alpha))
    return (np.clip(e.astype(np.float64), 0.0, 1.0) * 255.0).astype(np.uint8)
