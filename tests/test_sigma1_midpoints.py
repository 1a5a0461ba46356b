"""The extract path's sigma_1 enclosure next to float midpoints, on the CPU: the
fixtures tests/golden/sigma1_midpoints_b<b>.npz (tools/exp/sigma1_midpoints.py) hold what they
say -- every stored class follows from the frame alone -- and the numpy restatement of
sigma1_certified's f64 tail (tests/sigma1_helpers.py) has the kernel's margins: about 640 units of
2^-53 sigma_1 either side.  The GPU run is tests/test_sigma1_midpoints_gpu.py."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sigma1_helpers as S  # noqa: E402

BLOCKS = (4, 6, 8, 10, 12, 14, 16)
GRID = (4, 16)


def _fixture(b):
    return np.load(os.path.join(ROOT, "tests", "golden", f"sigma1_midpoints_b{b}.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def classes():
    """classify_frame of every fixture, computed once"""
    return {b: S.classify_frame(_fixture(b)["frame"], b) for b in BLOCKS}


def test_midpoint_distance():
    one = np.float32(1.0)
    up = np.nextafter(one, np.float32(2.0))
    m = (float(one) + float(up)) / 2.0
    assert S.midpoint_distance(m) == 0.0
    assert S.midpoint_distance(float(one)) == 2.0 ** 29 and S.midpoint_distance(float(up)) == 2.0 ** 29 / float(up)  # half a float spacing
    for scale in (2.0 ** -9, 0.5, 1.0, 2.0 ** 11):
        for r in (1.0, 37.0, 599.0, 640.0, 20480.0):
            for sign in (-1.0, 1.0):
                s = scale * m * (1.0 + sign * r * S.U)
                assert abs(S.midpoint_distance(s) - r) <= 2.0, (scale, r, sign)  # two f64 roundings built s, a unit each at most
    assert S.midpoint_distance(0.0) == np.inf
    x = np.random.default_rng(1).random(1000) * 4000.0 + 1e-3
    d = S.midpoint_distance(x)
    assert ((d >= 0.0) & (d <= 2.0 ** 29)).all()
    lo, hi = (x * (1.0 - d * S.U * 0.999)).astype(np.float32), (x * (1.0 + d * S.U * 0.999)).astype(np.float32)
    assert np.array_equal(lo, hi)  # no midpoint nearer than the distance says ...
    lo, hi = (x * (1.0 - (d + 2.0) * S.U)).astype(np.float32), (x * (1.0 + (d + 2.0) * S.U)).astype(np.float32)
    assert (lo != hi).all()  # ... and one at it


def test_tail_is_the_kernels():
    """The f64 tail restated in sigma1_helpers.tail is sigma1_certified's, constant for constant."""
    with open(os.path.join(ROOT, "thatsmyface_amd", "csrc", "tmfwm_device.h")) as f:
        src = f.read()
    body = src[src.index("TMF_DEVI void sigma1_certified"):]
    for line in ("constexpr double u = 1.1102230246251565e-16;",
                 "const double rho = a / nv;",
                 "const double rr0 = __builtin_sqrt(rn2 / nv) * (1.0 + 16.0 * u) + 256.0 * u * F;",
                 "const double rr = rr0 * rr0;",
                 "const double rlo = rho * (1.0 - 256.0 * u);",
                 "const double fhi = F * (1.0 + 256.0 * u);",
                 "const double gap = (rlo + rlo) - fhi;",
                 "const double hi = (rho + rr / (gap > 0.0 ? gap : 1.0)) * (1.0 + 256.0 * u);",
                 "const double slo = __builtin_sqrt(rlo) * (1.0 - 512.0 * u);",
                 "const double shi = __builtin_sqrt(hi) * (1.0 + 512.0 * u);",
                 "s1[m] = F == 0.0 ? 0.0f : (float)slo;",
                 "ok[m] = F == 0.0 || (gap > 0.0 && (float)shi == (float)slo && rho == rho);",
                 "const bool live = nn > 1e-30f;"):
        assert line in body, line
    passes = open(os.path.join(ROOT, "thatsmyface_amd", "csrc", "tmfwm_passes.h")).read()
    assert re.search(r"constexpr int kPowerIters = 3;", passes) and re.search(rf"constexpr int kListPowerIters = {S.LIST_ITERS};", passes)
    assert S.U == 1.1102230246251565e-16 and S.HALF_WIDTH == 512 + 256 / 2 and S.REFUSE == S.HALF_WIDTH - 40


@pytest.mark.parametrize("b", BLOCKS)
def test_stored_classes_follow_from_the_frame(classes, b):
    fx = _fixture(b)
    frame = fx["frame"]
    assert frame.dtype == np.uint8 and frame.shape == (GRID[0] * b, GRID[1] * b, 3) and int(fx["block"]) == b
    cls, dist, _ = classes[b]
    assert np.array_equal(np.argwhere(cls == S.MUST_REFUSE), fx["refuse"])
    assert np.array_equal(np.argwhere(cls == S.MUST_KEEP), fx["keep"])
    assert (cls != S.NONE).all()  # every other block is a fill block
    assert np.array_equal(dist[tuple(fx["refuse"].T)], fx["refuse_units"]) and np.array_equal(dist[tuple(fx["keep"].T)], fx["keep_units"])
    ru, ku = fx["refuse_units"], fx["keep_units"]
    assert len(ru) >= 6 and (ru > 200.0).sum() >= 2 and (ru < S.REFUSE).all()
    assert len(ku) >= 12 and ((ku >= S.REFUSE) & (ku <= S.KEEP_MAX)).all()
    assert len(fx["refuse_photo"]) == len(ru)
    assert int(fx["blocks_searched"]) >= 2_000_000
    # both halves of the frame hold must-refuse blocks (the ragged tests cut the top half off)
    top = int((fx["refuse"][:, 0] < GRID[0] // 2).sum())
    assert 2 <= top <= len(ru) - 2
    # no listed block within the last bits' reach of a class bound
    for u in np.concatenate([ru, ku]):
        assert min(abs(u - S.REFUSE), abs(u - S.KEEP_MAX)) >= 8.0
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", f"sigma1_midpoints_b{b}.npz")) <= 50_000


def test_a_photo_cover_block_is_among_the_must_refuse_ones():
    assert sum(bool(_fixture(b)["refuse_photo"].any()) for b in BLOCKS) >= 1


@pytest.mark.parametrize("b", BLOCKS)
def test_model_half_width_is_the_kernels_margin(classes, b):
    """512 u on the square root and half of 256 u under it, plus the residual term: the model's
    enclosure of every fixture block is 600 to 700 units wide either side after the list pass's
    iterations.  A kernel whose margins change needs another REFUSE bound."""
    cls, dist, half = classes[b]
    print(f"b={b}: half-width {half.min():.1f} .. {half.max():.1f} units on the listed blocks and fill")
    listed = cls != S.FILL
    assert ((half[listed] >= 600.0) & (half[listed] <= 700.0)).all(), (half[listed].min(), half[listed].max())
    # the model's own decisions on the listed blocks: none of the must-refuse ones, all must-keep ones
    fr = S.frame_blocks(_fixture(b)["frame"], b)
    ok = S.enclosure(fr, S.LIST_ITERS)[2].reshape(cls.shape)
    assert not ok[cls == S.MUST_REFUSE].any() and ok[cls != S.MUST_REFUSE].all()
    # and LAPACK's sigma_1 lies inside the enclosure, with at least 600 units either side
    slo, shi, _ = S.enclosure(fr, S.LIST_ITERS)
    s = S.sigma1_lapack(fr)
    assert ((s - slo >= 600.0 * S.U * s) & (shi - s >= 600.0 * S.U * s)).all()


def _midpoint_sweep():
    """sigma = m (1 +- r 2^-53) around float midpoints m, r from on the midpoint to far outside
    the margins, over the exponents sigma_1 of a DCT block can take."""
    rng = np.random.default_rng(53)
    f = np.concatenate([np.ldexp(1.0 + rng.random(4000), rng.integers(-12, 13, 4000)).astype(np.float32),
                        np.float32([1.0, 2.0, 1024.0, 1.9999999, 4095.9998])])
    m = (f.astype(np.float64) + np.nextafter(f, np.float32(np.inf)).astype(np.float64)) / 2.0
    r = np.array([0.0, 1.0, 100.0, 400.0, 599.0, 701.0, 1000.0, 5000.0, 1.0e5, 2.0 ** 28])
    sigma = np.concatenate([m[:, None] * (1.0 + r[None, :] * S.U), m[:, None] * (1.0 - r[None, :] * S.U)])
    return sigma, np.tile(r, (2 * len(m), 1))


def test_tail_alone_decides_by_the_distance():
    """A 1 x 1 'block' sigma with its exact vector: zero residual, rho = sigma^2.  The tail is
    undecided inside 600 units of a midpoint and decided outside 700."""
    sigma, r = _midpoint_sweep()
    x = sigma.reshape(-1, 1, 1)
    slo, shi, F, gap, rho = S.tail(x, np.ones((len(x), 1)))
    ok = S.decides(slo, shi, F, gap, rho).reshape(sigma.shape)
    assert (gap > 0.0).all()
    assert not ok[r < 600.0].any()
    assert ok[r > 700.0].all()
    half = (0.5 * (shi - slo) / (sigma.ravel() * S.U))
    assert ((half >= 636.0) & (half <= 644.0)).all(), (half.min(), half.max())
    # decided means: both ends, and sigma between them, round to the float the kernel returns
    s32 = slo.astype(np.float32).reshape(sigma.shape)
    assert np.array_equal(s32[ok], sigma.astype(np.float32)[ok])
    # with the 512 u of the square roots gone the same sweep decides at 400 units: the sweep is sharp
    c, h = 0.5 * (slo + shi), 0.5 * (shi - slo) - 512.0 * S.U * sigma.ravel()
    trimmed = S.decides(c - h, c + h, F, gap, rho).reshape(sigma.shape)
    assert trimmed[r == 400.0].any()
    # a zero block is decided as +0, a block with 2 rho <= F (two equal singular values) never
    z = S.enclosure(np.zeros((1, 4, 4), np.float32), 8)
    assert z[2][0]
    assert not S.enclosure(np.eye(4, dtype=np.float32)[None] * 3.0, 8)[2][0]


def test_byte_edge_sweep_is_sharp():
    """The points of tests/test_extract_byte_gpu.py: at least 200 of them change their byte when the
    quotient is computed as a product with 1 / alpha32, and every byte value is met at every alpha."""
    from keyed_helpers import bytes_of

    changed = 0
    for alpha in S.BYTE_ALPHAS:
        d = S.byte_edge_points(alpha)
        assert d.dtype == np.float32 and len(d) == 7 * 255 + 14
        exp = bytes_of(np.zeros_like(d), -d, alpha)
        assert set(exp[: 7 * 255]) == set(range(256)), alpha
        a32 = np.float32(alpha)
        at = {float(x): int(e) for x, e in zip(d, exp)}
        assert at[float(a32)] == 255 and at[float(np.nextafter(a32, np.float32(0)))] == 254 and at[float(np.nextafter(a32, 2 * a32))] == 255
        assert at[float(np.float32(3e38) * np.sign(a32))] == 255 and at[float(np.float32(-3e38) * np.sign(a32))] == 0
        assert at[float(np.float32(1e-45) * np.sign(a32))] == 0 and at[0.0] == 0
        changed += int((exp != S.byte_by_reciprocal(d, alpha)).sum())
    assert changed >= 200, changed
