"""Inputs that run every reachable branch of the dgesdd route -- test infrastructure only.

The cover corpora of the other tests (DCT blocks of images) all look alike: a dominant
positive D[0,0], moderate scale, no exact structure.  They never enter dbdsqr's zero-shift
sweep from the bottom, dlartg's scaled branch or dlasv2's ga >> fa branch.  This module
builds, on the CPU and from a seed alone,

  matrices(b, seed)                 general f32 blocks (structure, rank, scale, signed zeros)
  bidiagonals(b, seed)              upper-bidiagonal f32 blocks: dgebd2 leaves them as they are
                                    (zeros below the diagonal and right of the superdiagonal give
                                    tau = 0), so (d, e) reach dbdsqr exactly as written here
  pattern_cover(b, nbh, nbw, seed)  a uint8 RGB frame, one pixel pattern per block (line art,
                                    screenshots): these reach the zero-shift sweeps through embed
                                    and extract
  pattern_tile(nbh, nbw, seed)      a watermark tile with bytes 0, 255 and random bytes

each with one class label per block.  tools/lp_coverage.py measures what they reach in
oracle/tmfwm_lapack.c; tests/test_lp_corpus.py and tests/test_lp_corpus_gpu.py compare numpy,
the oracle, the host-compiled device header and the GPU on them.
"""
from __future__ import annotations

import itertools

import numpy as np

ALL_B = (4, 6, 8, 10, 12, 14, 16)
F32_TINY = float(np.finfo(np.float32).tiny)  # 2^-126, the smallest normal
F32_DENORM = 2.0 ** -149


def _f32(a) -> np.ndarray:
    with np.errstate(over="raise"):
        return np.ascontiguousarray(np.asarray(a, dtype=np.float64).astype(np.float32))


def _orth(rng, n) -> np.ndarray:
    q, r = np.linalg.qr(rng.standard_normal((n, n)))
    return q * np.sign(np.diag(r))


def _with_spectrum(rng, s) -> np.ndarray:
    n = len(s)
    return (_orth(rng, n) * np.asarray(s, np.float64)) @ _orth(rng, n).T


def _sylvester(n) -> np.ndarray:
    """+-1 entries (-1)^popcount(i & j): a Hadamard matrix where n is a power of two, its
    leading n x n corner (Hadamard-like, not orthogonal) elsewhere."""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    return 1.0 - 2.0 * (np.vectorize(lambda v: bin(v).count("1"))(i & j) & 1)


# ------------------------------------------------------------------------------------------------
# general matrices
# ------------------------------------------------------------------------------------------------
def _general(n, rng):
    """tests/test_oracle_lapack.py::_matrices' classes (8 draws of each random one)."""
    yield "eye", np.eye(n)
    yield "neg_eye", -np.eye(n)
    yield "diag_perm", np.diag(rng.permutation(n).astype(float))
    yield "diag_repeated", np.diag(np.repeat([3.0, 1.0], (n + 1) // 2)[:n])
    yield "perm_scaled", np.eye(n)[rng.permutation(n)] * 2.0
    yield "zero", np.zeros((n, n))
    for _ in range(8):
        yield "dense", rng.standard_normal((n, n))
        a = np.outer(rng.standard_normal(n), rng.standard_normal(n))
        a[rng.random((n, n)) < 0.1] = 0
        yield "rank1_sparse", a
        a = np.zeros((n, n))
        k = rng.integers(1, n + 1)
        a[rng.integers(0, n, k), rng.integers(0, n, k)] = rng.choice([-2.0, -1.0, 0.5, 1.0, 2.0], k)
        yield "single_entries", a
        yield "small_int", rng.integers(-2, 3, (n, n)).astype(np.float64)
        yield "binary_255", rng.integers(0, 2, (n, n)).astype(np.float64) * 255
        yield "repeated_rows", np.tile(rng.standard_normal(n), (n, 1))


def _structured(n, rng):
    # signs of the leading entry and of the whole spectrum
    a = np.abs(rng.standard_normal((n, n)))
    a[0, 0] = -50.0 * n
    yield "neg_leading", a
    a = rng.standard_normal((n, n))
    a[0, 0] = -abs(a[0, 0])
    yield "neg_leading", a
    yield "neg_definite_diag", -np.diag(np.sort(rng.random(n) + 0.1)[::-1])
    yield "neg_definite_diag", -np.diag(rng.random(n) + 0.1)
    yield "neg_definite", -(lambda g: g @ g.T)(rng.standard_normal((n, n)))
    # zero rows and columns: dlarfg's tau = 0, dlarf's trimming (iladlc / iladlr)
    for rows, cols in (((0,), ()), ((n - 1,), ()), ((), (0,)), ((), (n - 1,)), ((1, n - 2), ()), ((), (1, n - 2)),
                       ((0,), (0,)), ((n - 1,), (n - 1,)), (tuple(range(n // 2, n)), ()), ((), tuple(range(n // 2, n))),
                       (tuple(range(0, n // 2)), ()), ((), tuple(range(0, n // 2))),
                       (tuple(range(1, n)), ()), ((), tuple(range(1, n))), (tuple(range(2, n)), tuple(range(2, n)))):
        a = rng.standard_normal((n, n))
        a[list(rows), :] = 0
        a[:, list(cols)] = 0
        yield "zero_rows" if rows and not cols else "zero_cols" if cols and not rows else "zero_rows_cols", a
    for _ in range(3):
        a = rng.standard_normal((n, n))
        a[rng.random(n) < 0.4, :] = 0
        a[:, rng.random(n) < 0.4] = 0
        yield "zero_rows_cols", a
    for _ in range(2):
        yield "upper_triangular", np.triu(rng.standard_normal((n, n)))
        yield "lower_triangular", np.tril(rng.standard_normal((n, n)))
        yield "upper_triangular", np.triu(np.ones((n, n))) * rng.integers(1, 256)
        yield "lower_triangular", np.tril(np.ones((n, n))) * rng.integers(1, 256)
        yield "hessenberg", np.triu(rng.standard_normal((n, n)), -1)
    for _ in range(3):
        yield "orthogonal", _orth(rng, n) * 2.0 ** rng.integers(-6, 7)
    yield "orthogonal", np.eye(n)[::-1].copy()
    yield "hadamard_like", _sylvester(n)
    yield "hadamard_like", -_sylvester(n)
    yield "hadamard_like", _sylvester(n)[rng.permutation(n)] * 255.0
    yield "hadamard_like", rng.choice([-1.0, 1.0], (n, n))
    for r in range(1, n):
        yield f"rank_{r}", rng.standard_normal((n, r)) @ rng.standard_normal((r, n))
        yield f"rank_{r}", rng.integers(-3, 4, (n, r)).astype(float) @ rng.integers(-3, 4, (r, n)).astype(float)
    # graded spectra, both directions, and clusters
    for g in (1, 3, 8):
        s = 2.0 ** (-g * np.arange(n))
        yield "graded_spectrum_down", _with_spectrum(rng, s)
        yield "graded_spectrum_up", _with_spectrum(rng, s[::-1])
        d = np.diag(s)
        yield "graded_rows_down", d @ rng.standard_normal((n, n))
        yield "graded_rows_up", d[::-1, ::-1] @ rng.standard_normal((n, n))
        yield "graded_cols_down", rng.standard_normal((n, n)) @ d
        yield "graded_cols_up", rng.standard_normal((n, n)) @ d[::-1, ::-1]
        yield "graded_both", d @ rng.standard_normal((n, n)) @ d[::-1, ::-1]
        yield "graded_diag_up", np.diag(s[::-1])
    for eps in (1e-3, 1e-6, 0.0):
        s = np.concatenate([1.0 + eps * rng.random(n // 2), 1e-3 * (1.0 + eps * rng.random(n - n // 2))])
        yield "cluster", _with_spectrum(rng, s)
        yield "cluster", _with_spectrum(rng, 1.0 + eps * rng.random(n))
    # scale: f32 denormals up to ~1e30 (1e30 * sigma_1 stays below the f32 maximum), mixed rows
    for sc in (F32_DENORM, 8 * F32_DENORM, 1e-42, F32_TINY, 1e-30, 1e-20, 1e-10, 1e10, 1e20, 1e30):
        yield "scale_%.0e" % sc, rng.standard_normal((n, n)) * sc
        yield "scale_%.0e" % sc, rng.integers(-2, 3, (n, n)) * sc
    for _ in range(4):
        yield "mixed_scale_rows", rng.standard_normal((n, n)) * 10.0 ** rng.integers(-30, 31, (n, 1))
        yield "mixed_scale_cols", rng.standard_normal((n, n)) * 10.0 ** rng.integers(-30, 31, (1, n))
        yield "mixed_scale_entries", rng.standard_normal((n, n)) * 10.0 ** rng.integers(-40, 31, (n, n))
    # signed zeros
    yield "neg_zero", np.full((n, n), -0.0)
    yield "neg_zero", np.diag(np.full(n, -0.0)) + np.triu(np.ones((n, n)), 1) * -0.0
    for _ in range(4):
        a = rng.standard_normal((n, n))
        a[rng.random((n, n)) < 0.5] = -0.0
        yield "neg_zero", a
        a = np.where(rng.random((n, n)) < 0.5, -0.0, 0.0)
        a[rng.integers(0, n), rng.integers(0, n)] = rng.choice([-1.0, 1.0])
        yield "neg_zero", a
        a = np.diag(rng.choice([-0.0, 0.0, 1.0, -1.0], n))
        yield "neg_zero", np.where(np.eye(n) > 0, a, -0.0)


def matrices(b: int, seed: int = 0):
    """(n, b, b) float32 blocks and a list of n class labels."""
    rng = np.random.default_rng([int(seed), int(b), 1])
    labels, blocks = zip(*itertools.chain(_general(b, rng), _structured(b, rng)))
    return _f32(np.stack(blocks)), list(labels)


# ------------------------------------------------------------------------------------------------
# upper-bidiagonal blocks
# ------------------------------------------------------------------------------------------------
def _bidiag(d, e) -> np.ndarray:
    return np.diag(np.asarray(d, np.float64)) + np.diag(np.asarray(e, np.float64), 1)


def _pieces(n, size, vals):
    """Blocks whose (d, e) are consecutive `size` x `size` pieces split by zeros in e; vals is an
    iterable of per-piece tuples (d_1, e_1, d_2[, e_2, d_3]); the last block is padded with ones."""
    vals = list(vals)
    per = n // size
    for k in range(0, len(vals), per):
        d, e = np.ones(n), np.zeros(n - 1)
        for p, v in enumerate(vals[k:k + per]):
            o = p * size
            d[o:o + size] = v[0::2]
            e[o:o + size - 1] = v[1::2]
        yield _bidiag(d, e)


def _bidiagonal_blocks(n, rng):
    # trailing 2 x 2 pieces [f g; 0 h]: every ordering and zero case of dlasv2 (|f| <> |h|, g = 0,
    # |g| above and far above |f|, |h| above and below one in that branch, f = h ties)
    mags = (0.0, 1e-25, 0.5, 1.0, 2.0, 1e25)
    trip = [t for t in itertools.product(mags, repeat=3)]
    sgn = rng.choice([-1.0, 1.0], (len(trip), 3))
    trip = [tuple(np.array(t) * s) for t, s in zip(trip, sgn)]
    trip += [tuple(np.array(t) * s) for t in ((1.0, 2.0, 0.5), (0.5, 2.0, 1.0), (1.0, 0.25, 1.0), (3.0, 1e30, 2.0))
             for s in itertools.product((-1.0, 1.0), repeat=3)]
    trip += [(F32_DENORM, 1e30, F32_DENORM), (1e30, F32_DENORM, 1e30), (-F32_DENORM, 1.0, 1e30), (1.0, 1e-30, 1.0),
             (1e-30, 1e-30, 1e-30), (2.0, 1e-20, 2.0), (1e-20, 1.0, 1e20), (1e20, 1.0, 1e-20)]
    for a in _pieces(n, 2, trip):
        yield "pieces_2x2", a
    # one trailing 2 x 2 piece below a generic leading part
    for t in trip[:: max(1, len(trip) // 12)]:
        d, e = rng.standard_normal(n), rng.standard_normal(n - 1)
        d[n - 2], e[n - 2], d[n - 1] = t
        e[n - 3] = 0.0
        yield "trailing_2x2", _bidiag(d, e)
    # 3 x 3 pieces: the shift's dlas2 on well-conditioned pieces (|g| below and above max(|f|, |h|),
    # |f| <> |h|), and ill-conditioned ones (zero shift)
    rows = []
    for _ in range(40):
        v = rng.choice([-1.0, 1.0], 5) * 2.0 ** rng.uniform(-2, 2, 5)
        rows.append(tuple(v))
    for m in itertools.product((1e-3, 1.0, 1e3), repeat=5):
        rows.append(tuple(np.array(m) * rng.choice([-1.0, 1.0], 5)))
    for z in range(5):  # one exact zero in each position
        v = rng.standard_normal(5)
        v[z] = 0.0
        rows.append(tuple(v))
    for a in _pieces(n, 3, rows):
        yield "pieces_3x3", a
    # unreduced blocks, both chase directions: |d[ll]| above and below |d[m]|, mild to strong grading
    for g in (0.0, 0.25, 1.0, 3.0, 8.0, 20.0):
        for _ in range(3):
            s = 2.0 ** (-g * np.arange(n))
            d, e = s * rng.choice([-1.0, 1.0], n) * rng.uniform(0.5, 1.0, n), rng.standard_normal(n - 1)
            yield "graded_down", _bidiag(d, e * s[1:])
            yield "graded_down", _bidiag(d, e * s[:-1])
            yield "graded_up", _bidiag(d[::-1], (e * s[1:])[::-1])
            yield "graded_up", _bidiag(d[::-1], (e * s[:-1])[::-1])
    for sc in (F32_DENORM * 2 ** 10, 1e-30, 1e-10, 1e10, 1e30):
        yield "scaled", _bidiag(rng.standard_normal(n), rng.standard_normal(n - 1)) * sc
        yield "scaled", _bidiag(np.sort(rng.random(n) + 0.1), rng.standard_normal(n - 1)) * sc
    for _ in range(4):
        yield "mixed_scale", _bidiag(rng.standard_normal(n) * 10.0 ** rng.integers(-30, 31, n),
                                     rng.standard_normal(n - 1) * 10.0 ** rng.integers(-30, 31, n - 1))
        yield "huge_offdiag", _bidiag(rng.standard_normal(n), rng.standard_normal(n - 1) * 1e20)
        yield "tiny_offdiag", _bidiag(rng.standard_normal(n), rng.standard_normal(n - 1) * 1e-20)
    # every entry at its own extreme of the f32 range, some zero: sigma_min far below the f32
    # range keeps dbdsqr's thresholds tiny, so off-diagonal entries survive down to |g / f| < 2^-537,
    # where dlasv2's (g / f)^2 underflows to zero (its mm = 0 branch)
    for _ in range(150):
        ex = rng.choice([-149, -140, -100, -50, 0, 50, 100, 127], 2 * n - 1) + rng.integers(-3, 1, 2 * n - 1)
        v = rng.choice([-1.0, 1.0], 2 * n - 1) * 2.0 ** np.clip(ex, -149, 127)
        v[rng.random(2 * n - 1) < 0.05] = 0.0
        yield "extreme", _bidiag(v[:n], v[n:])
    # zero diagonal entries: the zero-diagonal chase (first, inner, last, several, all)
    for zs in ((0,), (n - 1,), (n // 2,), (1,), (n - 2,), (0, n - 1), (1, n // 2), tuple(range(0, n, 2)), tuple(range(1, n, 2)),
               tuple(range(n))):
        for up in (False, True):
            d, e = np.sort(rng.random(n) + 0.5), rng.standard_normal(n - 1)
            d = d if up else d[::-1].copy()
            d[list(zs)] = 0.0
            yield "zero_diag", _bidiag(d, e)
    yield "zero_diag", _bidiag(np.zeros(n), np.ones(n - 1))
    yield "zero_diag", _bidiag(np.full(n, -0.0), -np.ones(n - 1))
    # negative d (the sign flip) and ties (the three selection sorts)
    for _ in range(3):
        yield "negative_d", _bidiag(-np.abs(rng.standard_normal(n)), rng.standard_normal(n - 1))
        yield "negative_d", _bidiag(-np.sort(rng.random(n) + 0.1), np.zeros(n - 1))
        yield "ties", _bidiag(rng.choice([-1.0, 1.0], n), np.zeros(n - 1))
        yield "ties", _bidiag(rng.choice([1.0, 2.0, 3.0], n) * rng.choice([-1.0, 1.0], n), np.zeros(n - 1))
        yield "ties", _bidiag(rng.choice([0.0, -0.0, 1.0, -1.0], n), np.zeros(n - 1))
        yield "ties", _bidiag(np.ones(n), np.full(n - 1, 2.0 ** -rng.integers(1, 40)))
        yield "ties", _bidiag(rng.choice([1.0, 2.0], n), rng.choice([0.0, 0.5], n - 1))
    yield "ties", _bidiag(np.ones(n), np.ones(n - 1))
    yield "ties", _bidiag(np.arange(1, n + 1), np.zeros(n - 1))
    yield "ties", _bidiag(np.arange(n, 0, -1), np.zeros(n - 1))
    yield "ties", _bidiag(-np.ones(n), np.ones(n - 1))


def bidiagonals(b: int, seed: int = 0):
    """(n, b, b) float32 upper-bidiagonal blocks and a list of n class labels."""
    rng = np.random.default_rng([int(seed), int(b), 2])
    labels, blocks = zip(*_bidiagonal_blocks(b, rng))
    D = _f32(np.stack(blocks))
    assert not np.tril(D, -1).any() and not np.triu(D, 2).any()
    return D, list(labels)


def rescale_sigma1(D: np.ndarray, seed: int = 0, lo: int = -8, hi: int = 4) -> np.ndarray:
    """The same blocks scaled by powers of two (exact) so that sigma_1 lies in [2^lo, 2^hi], the
    range of pixel DCT blocks; zero blocks stay zero.  Elements that a block's own dynamic range
    pushes below the f32 normal range are dropped to zero rather than rounded to denormals."""
    rng = np.random.default_rng([int(seed), 3])
    out = np.zeros_like(D)
    for k, a in enumerate(D.astype(np.float64)):
        amax = np.abs(a).max()
        if amax == 0.0:
            continue
        a = a * 2.0 ** -np.floor(np.log2(amax))  # exact: max |a| in [1, 2)
        s1 = np.linalg.svd(a, compute_uv=False)[0]
        t = rng.integers(lo, hi)  # target sigma_1 in [2^t, 2^(t+1))
        a = a * 2.0 ** (t - np.floor(np.log2(s1)))
        a[np.abs(a) < F32_TINY] = 0.0
        out[k] = a
    return out


# ------------------------------------------------------------------------------------------------
# pattern covers
# ------------------------------------------------------------------------------------------------
def _masks(b, rng):
    """name -> a (b, b) float mask in [0, 1]: 0 = background colour, 1 = foreground colour."""
    i, j = np.meshgrid(np.arange(b), np.arange(b), indexing="ij")
    r, c = rng.integers(0, b), rng.integers(0, b)
    perm = rng.permutation(b)
    lev = rng.permutation(b)
    u, v = rng.integers(0, 2, b), rng.integers(0, 2, b)
    u2, v2 = rng.integers(0, 2, b), rng.integers(0, 2, b)
    w = rng.integers(1, max(2, b // 4) + 1)
    return {
        # the twelve simple patterns
        "hline": (i == r) * 1.0,
        "vline": (j == c) * 1.0,
        "diagonal": (i == j) * 1.0,
        "checker1": ((i + j) & 1) * 1.0,
        "checker2": (((i >> 1) + (j >> 1)) & 1) * 1.0,
        "permutation": (j == perm[i]) * 1.0,
        "triangle_lower": (i >= j) * 1.0,
        "triangle_upper": (i <= j) * 1.0,
        "graded_rows": 0.5 ** lev[i],
        "graded_cols": 0.5 ** lev[j],
        "ramp": j / (b - 1.0),
        "ramp_diag": (i + j) / (2.0 * b - 2.0),
        # further families
        "lowrank_two_level": np.outer(u, v) * 1.0,
        "lowrank_two_level2": np.clip(np.outer(u, v) + np.outer(u2, v2), 0, 1) * 1.0,
        "border": ((i < w) | (j < w) | (i >= b - w) | (j >= b - w)) * 1.0,
        "cross": ((i == r) | (j == c)) * 1.0,
        "antidiagonal": (i + j == b - 1) * 1.0,
    }


PATTERNS = tuple(_masks(4, np.random.default_rng(0)))


def pattern_cover(b: int, nbh: int = 24, nbw: int = 24, seed: int = 0, edge_rows: int = 3, edge_cols: int = 5):
    """A (nbh * b + edge_rows, nbw * b + edge_cols, 3) uint8 frame, one pattern per block, every
    block with its own random background and foreground colour (R, G and B differ), and random
    edge pixels; and the (nbh, nbw) array of pattern names."""
    rng = np.random.default_rng([int(seed), int(b), 4])
    H, W = nbh * b + edge_rows, nbw * b + edge_cols
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    names = np.empty((nbh, nbw), dtype=object)
    order = rng.permutation(nbh * nbw)
    for q, k in enumerate(order):
        bi, bj = divmod(int(k), nbw)
        masks = _masks(b, rng)
        name = PATTERNS[q % len(PATTERNS)]
        bg, fg = rng.integers(0, 256, 3), rng.integers(0, 256, 3)
        if q % 5 == 0:  # pure black / white line art
            bg, fg = (np.zeros(3), np.full(3, 255)) if q % 10 else (np.full(3, 255), np.zeros(3))
        m = masks[name][..., None]
        img[bi * b:(bi + 1) * b, bj * b:(bj + 1) * b] = np.floor(bg + (fg - bg) * m + 0.5).astype(np.uint8)
        names[bi, bj] = name
    return img, names


def sparse_pattern_cover(b: int, nbh: int = 24, nbw: int = 24, seed: int = 0, rows: int = 2):
    """pattern_cover's first `rows` block rows on top of a noise frame of the same size: few
    enough blocks go to the dgesdd route (under an eighth) that the second pass of the hybrid
    route gives each of them a whole wave instead of a group of lanes."""
    img, names = pattern_cover(b, nbh, nbw, seed)
    out = np.random.default_rng([int(seed), int(b), 6]).integers(0, 256, img.shape, dtype=np.uint8)
    out[: rows * b, : nbw * b] = img[: rows * b, : nbw * b]
    return out, names[:rows]


def pattern_tile(nbh: int, nbw: int, seed: int = 0) -> np.ndarray:
    """(nbh, nbw) uint8 watermark bytes: a third 0, a third 255, a third random."""
    rng = np.random.default_rng([int(seed), 5])
    t = rng.integers(0, 256, (nbh, nbw), dtype=np.uint8)
    k = rng.integers(0, 3, (nbh, nbw))
    t[k == 0] = 0
    t[k == 1] = 255
    return t


def cover_standin(b: int, noise_hw=(1080, 1920)):
    """The cover frames the GPU tests send through the dgesdd route, as (frame, tile) pairs: the
    structured cover classes at the tests' size and one noise frame (tools/lp_coverage.py)."""
    from golden.gen_golden import cover, wmark
    from lapack_path import photo_cover

    H, W = 272, 480
    out = []
    for kind in ("noise", "photo", "smooth", "blocky", "qr", "diagonal", "flat", "black"):
        c = photo_cover(H, W, 11) if kind == "photo" else np.ascontiguousarray(cover(kind, H, W, 11))
        out.append((c, wmark("qr", H // b, W // b, 3)))
    H, W = noise_hw
    rng = np.random.default_rng(90 + b)
    out.append((rng.integers(0, 256, (H, W, 3), dtype=np.uint8), rng.integers(0, 256, (H // b, W // b), dtype=np.uint8)))
    return out
