"""The f32 colour-tail decision of the embed kernels (thatsmyface_amd/csrc/tmfwm_colour_tail.h)
compiled for the host CPU (tests/native/colour_tail_host.cpp) and checked against the exact f64
tail, restated there from tmfwm_device.h: an accepted pixel's bytes are the exact tail's at Y's
lower end and at its upper end.  The GPU run of both tails is tests/test_colour_tail_gpu.py."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "colour_tail_host.cpp")
HDR = os.path.join(ROOT, "thatsmyface_amd", "csrc", "tmfwm_colour_tail.h")
OUT = os.path.join(ROOT, "tests", "_build", "libcolour_tail_host.so")
FLAGS = ["-O2", "-march=native", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fopenmp"]

# Y's lower end relative to the colour's own luma: the luma itself, then offsets of a fraction of
# a level up to several levels, both signs
OFFS = np.array([0.0] + [s * k / 255.0 for k in (0.31, 0.77, 1.52, 3.3, 7.9) for s in (1, -1)], np.float32)
# absolute lower ends: below 0 and above 1 (both clips), |Y| up to 8 (alpha at its edges)
ABSY = np.array([-8.0, -2.5, -1.0, -0.03, -1e-4, 0.0, 1.0, 1.0 + 1e-4, 1.03, 2.0, 3.7, 8.0], np.float32)
# solved lower ends: each channel's scaled value at a byte boundary + e * delta
SOLVE_FULL = np.array([-2.0, -1.5, -1.0, -0.75, -0.25, -0.01, 0.01, 0.25, 0.75, 1.0, 1.5, 2.0], np.float32)
SOLVE_QUICK = np.array([-2.0, -1.0, -0.25, 0.25, 1.0, 2.0], np.float32)


@pytest.fixture(scope="module")
def host():
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        tmp = f"{OUT}.{os.getpid()}.tmp"  # pytest-xdist workers may build at once: write aside, rename
        subprocess.run([cxx, *FLAGS, "-fPIC", "-shared", "-o", tmp, SRC], check=True)
        os.replace(tmp, OUT)
    L = ctypes.CDLL(OUT)
    fp = ctypes.c_void_p
    L.ct_sweep.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, fp, ctypes.c_int, fp, ctypes.c_int, fp, ctypes.c_int, fp]
    L.ct_accept_rate.argtypes = [ctypes.c_float, ctypes.c_float, fp]
    L.ct_fast.argtypes = [ctypes.c_uint32] * 3 + [ctypes.c_float, ctypes.c_float, fp]
    L.ct_delta.restype = ctypes.c_float
    return L


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _sweep(host, offs, absy, solve, step=1):
    out = np.zeros(6, np.int64)
    host.ct_sweep(0, 1 << 24, step, _p(offs), len(offs), _p(absy), len(absy), _p(solve), len(solve), _p(out))
    evals, accepted, bad = (int(x) for x in out[:3])
    per_colour = 4 * (len(offs) + len(absy) + 6 * len(solve))  # four widths dY per lower end
    assert evals == per_colour * len(range(0, 1 << 24, step))
    first = (hex(int(out[3])), np.uint32(out[4]).view(np.float32), np.uint32(out[5]).view(np.float32))
    assert bad == 0, f"{bad} accepted pixels with other bytes than the exact tail; first (colour, yl, dy) = {first}"
    return accepted / evals


def test_accepted_bytes_are_exact_all_colours(host):
    """All 2^24 byte triples, each at 35 lower ends (its luma, luma +- 5 offsets, 12 absolute
    values, each channel's 2 byte boundaries +- {0.25, 1, 2} delta) and 4 widths {0, 1 ulp, 2^-20,
    2^-12}: accepted => the bytes of colour_inv(yl) and of colour_inv(yh)."""
    rate = _sweep(host, OFFS, ABSY, SOLVE_QUICK[[1, 4]], step=1)
    assert 0.0 < rate < 1.0  # both outcomes occur: the sweep straddles the boundaries


@pytest.mark.slow
def test_accepted_bytes_are_exact_full_sweep(host):
    """The same over 95 lower ends per colour (12 solved offsets per boundary)."""
    _sweep(host, OFFS, ABSY, SOLVE_FULL, step=1)


def test_accept_rate_matches_the_bound(host):
    """Every colour once, Y's lower end within +-2 levels of the colour's luma, dY = 2^-22 (a
    certified block's interval width).  A channel that is not clipped rejects when its scaled
    value is within delta below or delta + 2^-14 + 2^-20 + 255.1 dY above a byte boundary: a share
    2 delta + 2^-14 + 2^-20 + 255.1 * 2^-22 = 3.37e-4 of a level (delta = 7 * 2^-16), so at most
    3 * 3.37e-4 = 1.01e-3 of the pixels reject and the accept rate is at least 0.99899.  A bound
    loosened by accident (delta doubled: 0.99835) fails the 0.9985 asserted here."""
    assert host.ct_delta() == np.float32(7 * 2.0**-16)
    out = np.zeros(3, np.int64)
    host.ct_accept_rate(2.0 / 255.0, 2.0**-22, _p(out))
    n, acc, bad = (int(x) for x in out)
    assert bad == 0
    rate = acc / n
    print(f"accept rate {rate:.6f} over {n} colours")
    assert rate >= 0.9985
    # point intervals (dY = 0): the share per channel is 2 delta + 2^-14 + 2^-20 = 2.76e-4
    host.ct_accept_rate(2.0 / 255.0, 0.0, _p(out))
    assert int(out[2]) == 0 and int(out[1]) / n >= 1.0 - 3 * 2.76e-4 - 1e-4


def test_non_finite_inputs_reject(host):
    rgb = np.zeros(3, np.uint32)
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    half = np.float32(0.5)
    # (yl, yh) with a non-finite end; the width the kernels pass is yh - yl (or 2 eps_Y around a
    # non-finite centre): non-finite as well
    for yl, yh in ((nan, nan), (nan, half), (half, nan), (inf, inf), (-inf, -inf), (-inf, inf), (-inf, half), (half, inf),
                   (inf, half)):
        with np.errstate(invalid="ignore"):
            dy = np.float32(yh) - np.float32(yl)
        for col in ((0, 0, 0), (255, 255, 255), (12, 200, 77)):
            assert host.ct_fast(*col, yl, dy, _p(rgb)) == 0, (yl, yh, col)
    # finite, far outside [0, 1]: decided by the clip
    assert host.ct_fast(12, 200, 77, 1e30, 0.0, _p(rgb)) == 1 and list(rgb) == [255, 255, 255]
    assert host.ct_fast(12, 200, 77, -1e30, 0.0, _p(rgb)) == 1 and list(rgb) == [0, 0, 0]


def test_grey_at_its_own_luma_rejects(host):
    """A block the watermark leaves alone (tile value 0) reproduces its source bytes.  The two
    colour matrices are inverses only to ~10^-3, so a saturated colour comes back well inside a
    level; a grey comes back on the byte boundary itself (each inverse row applied to the forward
    rows sums to 1), which the f32 path must leave to the exact tail."""
    rgb = np.zeros(3, np.uint32)
    for v in range(1, 256):
        unit = np.float32(v) / np.float32(255)
        y = np.float32(0.114 * float(unit) + (0.299 * float(unit) + 0.587 * float(unit)))
        assert host.ct_fast(v, v, v, y, 0.0, _p(rgb)) == 0, v
    out = np.zeros(3, np.int64)
    host.ct_accept_rate(0.0, 0.0, _p(out))  # every colour at its own luma: sound, mostly accepted
    assert int(out[2]) == 0 and int(out[1]) > (1 << 24) * 0.98


def test_standalone_under_sanitizers(tmp_path):
    """The stand-alone main of the same file (a strided sweep) under ASan + UBSan on the host."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "colour_tail_san"
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-DCT_MAIN",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", SRC, "-o",
                    str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1"))
    assert r.returncode == 0, r.stderr[-3000:]
    assert '"bad": 0' in r.stdout, r.stdout
