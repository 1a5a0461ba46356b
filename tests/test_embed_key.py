"""Embed that also returns the extraction key, on the CPU: the two entry points
exist and agree across the header, the library and the ctypes table; they validate their
arguments before any device work; the Python wrappers check key_out; and the kernels' key
decision (thatsmyface_amd/csrc/tmfwm_embed_key.h, compiled for the host from
tests/native/embed_key_host.cpp) decides exactly when both ends of sigma_1 round to one float --
and then every f64 between them rounds to the key.  The GPU run is tests/test_embed_key_gpu.py."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

from thatsmyface_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import embed_key_helpers as EK  # noqa: E402

SRC = os.path.join(ROOT, "tests", "native", "embed_key_host.cpp")
HDR = os.path.join(ROOT, "thatsmyface_amd", "csrc", "tmfwm_embed_key.h")
OUT = os.path.join(ROOT, "tests", "_build", "libembed_key_host.so")
NAMES = ("tmfwm_embed_key", "tmfwm_embed_key_ragged")
BLOCKS = (4, 6, 8, 10, 12, 14, 16)


def _p(x):
    return x.ctypes.data


def test_new_names_exist_and_agree():
    with open(os.path.join(ROOT, "include", "tmfwm.h")) as f:
        header = f.read()
    L = _lib.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for n in NAMES:
        assert re.search(r"\bint " + n + r"\s*\(", header), n
        assert n in _lib.SIGNATURES, n
        assert hasattr(L, n), n
        assert re.search(r" T " + n + r"\b", nm), n
    assert len(_lib.SIGNATURES["tmfwm_embed_key"][1]) == 16 and len(_lib.SIGNATURES["tmfwm_embed_key_ragged"][1]) == 8
    # the 40-byte frame: four pointers and two int32, in the header's order
    m = re.search(r"typedef struct \{([^}]*)\} tmfwm_embed_key_frame;", header)
    assert m, "tmfwm_embed_key_frame"
    fields = re.findall(r"\*?(\w+)\s*[;,]", re.sub(r"/\*.*?\*/", "", m.group(1)))
    assert fields == ["rgb", "out", "wm_tile", "out_key", "height", "width"], fields
    assert [f[0] for f in _lib.EmbedKeyFrame._fields_] == fields
    assert ctypes.sizeof(_lib.EmbedKeyFrame) == 40
    assert L.tmfwm_abi_version() == 10  # added within ABI 10


def test_argument_validation_before_device():
    L = _lib.load()
    a = np.zeros((2, 16, 16, 3), np.uint8)
    o = np.zeros_like(a)
    t = np.zeros((2, 2), np.uint8)
    k = np.zeros((2, 2, 2), np.float32)
    H = _lib.MEM_HOST
    kb = 2 * 2 * 4

    def emb(n=2, block=8, route=0, alpha=0.1, key_stride=kb, tile_stride=0):
        return L.tmfwm_embed_key(_p(a), n, 16, 16, 16 * 16 * 3, _p(t), tile_stride, block, alpha, _p(o), _p(k), key_stride, H, None,
                                 route, None)

    def rag(n=1, block=8, route=0, alpha=0.1):
        d = (_lib.EmbedKeyFrame * 1)(_lib.EmbedKeyFrame(_p(a), _p(o), _p(t), _p(k), 16, 16))
        return L.tmfwm_embed_key_ragged(ctypes.addressof(d), n, block, alpha, H, None, route, None)

    for bad_block in (7, 18, 2):
        with pytest.raises(NotImplementedError):
            _lib.check(emb(block=bad_block), "embed_key")
        with pytest.raises(NotImplementedError):
            _lib.check(rag(block=bad_block), "embed_key_ragged")
    for bad_route in (-1, 4):
        with pytest.raises(ValueError, match="route"):
            _lib.check(emb(route=bad_route), "embed_key")
        with pytest.raises(ValueError, match="route"):
            _lib.check(rag(route=bad_route), "embed_key_ragged")
    for rank1 in (_lib.ROUTE_RANK1, _lib.ROUTE_RANK1_REFERENCE):  # the ragged calls take no rank-1 route
        with pytest.raises(NotImplementedError):
            _lib.check(rag(route=rank1), "embed_key_ragged")
    with pytest.raises(ValueError, match="alpha"):
        _lib.check(emb(alpha=float("nan")), "embed_key")
    with pytest.raises(ValueError, match="alpha"):
        _lib.check(rag(alpha=float("nan")), "embed_key_ragged")
    for short in (kb - 4, 0, -16):  # a short key_stride
        with pytest.raises(ValueError, match="key_stride"):
            _lib.check(emb(key_stride=short), "embed_key")
    for odd in (kb + 2, kb + 1):  # not a multiple of 4
        with pytest.raises(ValueError, match="key_stride"):
            _lib.check(emb(key_stride=odd), "embed_key")
    with pytest.raises(ValueError, match="tile_stride"):
        _lib.check(emb(tile_stride=3), "embed_key")
    with pytest.raises(ValueError, match="negative"):
        _lib.check(emb(n=-1), "embed_key")
    with pytest.raises(ValueError, match="negative"):
        _lib.check(rag(n=-1), "embed_key_ragged")
    # a misaligned key pointer of a frame with a block (ragged: checked before the device is touched)
    d = (_lib.EmbedKeyFrame * 1)(_lib.EmbedKeyFrame(_p(a), _p(o), _p(t), _p(k) + 2, 16, 16))
    with pytest.raises(ValueError, match="out_key is not 4-byte aligned"):
        _lib.check(L.tmfwm_embed_key_ragged(ctypes.addressof(d), 1, 8, 0.1, H, None, 0, None), "embed_key_ragged")
    d = (_lib.EmbedKeyFrame * 1)(_lib.EmbedKeyFrame(_p(a), _p(o), _p(t), None, 16, 16))
    with pytest.raises(ValueError, match="NULL"):
        _lib.check(L.tmfwm_embed_key_ragged(ctypes.addressof(d), 1, 8, 0.1, H, None, 0, None), "embed_key_ragged")


@pytest.mark.skipif(_lib.device_count() > 0, reason="CPU-only check")
def test_fails_loudly_without_gpu():
    from thatsmyface_amd import watermarking as W

    L = _lib.load()
    a = np.zeros((1, 16, 16, 3), np.uint8)
    o = np.zeros_like(a)
    t = np.zeros((2, 2), np.uint8)
    k = np.zeros((2, 2), np.float32)
    with pytest.raises(_lib.TmfwmError, match="no HIP device"):
        # (key_stride is ignored for one frame)
        _lib.check(L.tmfwm_embed_key(_p(a), 1, 16, 16, a.size, _p(t), 0, 8, 0.1, _p(o), _p(k), 0, _lib.MEM_HOST, None, 0, None), "e")
    d = (_lib.EmbedKeyFrame * 1)(_lib.EmbedKeyFrame(_p(a), _p(o), _p(t), _p(k), 16, 16))
    with pytest.raises(_lib.TmfwmError, match="no HIP device"):
        _lib.check(L.tmfwm_embed_key_ragged(ctypes.addressof(d), 1, 8, 0.1, _lib.MEM_HOST, None, 0, None), "r")
    with pytest.raises(_lib.TmfwmError, match="no HIP device"):
        W.embed_watermark_with_key(Image.new("RGB", (16, 16)), Image.new("L", (8, 8)), custom_settings={"block_size": 8, "alpha": 0.1})


def test_python_wrappers_check_key_out():
    """Wrong shapes, dtypes and devices of key_out are refused before the library is called
    (CPU tensors stand in for the frames: the first check names them)."""
    torch = pytest.importorskip("torch")
    from thatsmyface_amd import batch
    from thatsmyface_amd import watermarking as W
    from thatsmyface_amd.modules import watermarking as M

    assert M.embed_watermark_with_key is W.embed_watermark_with_key
    with pytest.raises(ValueError, match="GPU tensor"):
        batch.embed_with_key(torch.zeros((1, 16, 16, 3), dtype=torch.uint8), torch.zeros((2, 2), dtype=torch.uint8), 8)
    with pytest.raises(NotImplementedError):
        batch.embed_with_key_ragged([], [], 7)
    with pytest.raises(NotImplementedError, match="rank-1"):
        batch.embed_with_key_ragged([], [], 8, route="rank1")
    assert batch.embed_with_key_ragged([], [], 8) == ([], [])
    with pytest.raises(ValueError, match="positive"):
        W.embed_watermark_with_key(Image.new("RGB", (16, 16)), Image.new("L", (8, 8)), custom_settings={"block_size": 0, "alpha": 0.1})
    if not torch.cuda.is_available():
        return
    dev = torch.device("cuda", 0)
    fr = torch.zeros((2, 16, 24, 3), dtype=torch.uint8, device=dev)
    tile = torch.zeros((2, 3), dtype=torch.uint8, device=dev)
    for bad in (torch.zeros((2, 2, 3), dtype=torch.float64, device=dev), torch.zeros((2, 3, 2), dtype=torch.float32, device=dev),
                torch.zeros((2, 3), dtype=torch.float32, device=dev), torch.zeros((2, 2, 3), dtype=torch.float32),
                torch.zeros((2, 2, 6), dtype=torch.float32, device=dev)[:, :, ::2]):
        with pytest.raises(ValueError, match="key_out"):
            batch.embed_with_key(fr, tile, 8, key_out=bad)
    good = torch.zeros((2, 3), dtype=torch.float32, device=dev)
    for bad in (good.double(), torch.zeros((3, 2), dtype=torch.float32, device=dev), good.cpu(),
                torch.zeros((2, 6), dtype=torch.float32, device=dev)[:, ::2], None):
        with pytest.raises(ValueError, match=r"out\[1\]"):
            batch.embed_with_key_ragged([fr[0], fr[1]], [tile, tile], 8, key_out=[good, bad])
    with pytest.raises(ValueError, match="one key per frame"):
        batch.embed_with_key_ragged([fr[0], fr[1]], [tile, tile], 8, key_out=[torch.zeros((2, 3), dtype=torch.float32, device=dev)])


# ---- the decision header on the host

@pytest.fixture(scope="module")
def host():
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        tmp = f"{OUT}.{os.getpid()}.tmp"  # pytest-xdist workers may build at once: write aside, rename
        subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Werror", "-fPIC", "-shared", "-o",
                        tmp, SRC], check=True)
        os.replace(tmp, OUT)
    L = ctypes.CDLL(OUT)
    vp = ctypes.c_void_p
    L.ek_decide.argtypes = [ctypes.c_float, ctypes.c_float, vp]
    L.ek_of.argtypes = [vp, vp, ctypes.c_longlong, vp, vp]
    L.ek_of.restype = None
    return L


def _of(host, sigma, tE):
    sigma = np.ascontiguousarray(sigma, np.float64)
    tE = np.ascontiguousarray(np.broadcast_to(tE, sigma.shape), np.float64)
    dec = np.zeros(sigma.shape, np.uint8)
    key = np.zeros(sigma.shape, np.float32)
    host.ek_of(_p(sigma), _p(tE), sigma.size, _p(dec), _p(key))
    return dec.astype(bool), key


def _midpoint_sweep():
    """sigma around float midpoints: m = (f + nextafter(f)) / 2 exactly in f64, sigma = m +- d for
    d = r * 2^-45 m, r below and above 1 (and 0: on the midpoint itself) -- floats f over the
    exponents a DCT block's sigma_1 can take (b = 4..16: up to 16 * 255/255 = 16) and beyond."""
    rng = np.random.default_rng(45)
    f = np.concatenate([np.ldexp(1.0 + rng.random(4000), rng.integers(-20, 8, 4000)).astype(np.float32),
                        np.float32([1.0, 2.0, 0.5, 16.0, 1.9999999, 3.9999998])])  # powers of two: the spacing changes there
    m = (f.astype(np.float64) + np.nextafter(f, np.float32(np.inf)).astype(np.float64)) / 2.0
    r = np.array([0.0, 0.25, 0.5, 0.9, 0.999, 1.001, 1.1, 2.0, 4.0, 1000.0])
    d = r[None, :] * (2.0 ** -45) * m[:, None]
    sigma = np.concatenate([(m[:, None] + d).ravel(), (m[:, None] - d).ravel()])
    return sigma, (2.0 ** -45) * sigma


def test_decided_iff_both_ends_round_to_one_float(host):
    sigma, tE = _midpoint_sweep()
    dec, key = _of(host, sigma, tE)
    lo, hi = (sigma - tE).astype(np.float32), (sigma + tE).astype(np.float32)
    assert np.array_equal(dec, lo == hi)
    assert dec.any() and (~dec).any()  # the sweep straddles the midpoints
    # well inside (r <= 0.25 of tE from the midpoint) is undecided, well outside (r >= 4) decided
    n = len(sigma) // 2
    for half in (slice(0, n), slice(n, 2 * n)):
        d = dec[half].reshape(-1, 10)
        assert not d[:, :2].any() and d[:, 8:].all()
    assert np.array_equal(key.view(np.uint32), lo.view(np.uint32))
    dn, kn = EK.decide(sigma, tE)  # the numpy restatement the GPU tests predict with
    assert np.array_equal(dn, dec) and np.array_equal(kn.view(np.uint32), key.view(np.uint32))


def test_decided_key_is_the_rounding_of_every_value_between_the_ends(host):
    sigma, tE = _midpoint_sweep()
    dec, key = _of(host, sigma, tE)
    lo, hi = sigma - tE, sigma + tE
    rng = np.random.default_rng(46)
    # the ends, the centre, the f64 neighbours just inside the ends, and random points between
    points = [lo, hi, sigma, np.nextafter(lo, np.inf), np.nextafter(hi, -np.inf)] + [lo + rng.random(len(lo)) * (hi - lo) for _ in range(8)]
    for x in points:
        x = np.clip(x, lo, hi)
        assert np.array_equal(x.astype(np.float32)[dec].view(np.uint32), key[dec].view(np.uint32))
    # ... among them LAPACK's sigma_1, which the certificate puts within tE of the Jacobi route's


def test_point_intervals_and_the_clamp(host):
    rng = np.random.default_rng(47)
    sigma = np.concatenate([[0.0, 5e-324, 1e-46, 2.0 ** -126, 2.0 ** -149, 1.0, 16.0, 255.0 * 16], rng.random(1000) * 40.0,
                            np.ldexp(rng.random(1000), rng.integers(-160, 12, 1000))])
    dec, key = _of(host, sigma, 0.0)
    assert dec.all()  # tE = 0 (zero, flat and flagged blocks): both ends are f32(sigma)
    assert np.array_equal(key.view(np.uint32), sigma.astype(np.float32).view(np.uint32))
    assert key[0] == 0.0 and not np.signbit(key[0])
    # tE > sigma: the lower end clamps at +0 (never a negative float)
    dec, key = _of(host, [1e-50, 1e-50, 0.0, 1.0], [1e-49, 1.0, 1e-60, 2.0])
    assert list(dec) == [True, False, True, False]
    assert (key.view(np.uint32) == 0).all()
    # non-finite ends decide nothing
    k = ctypes.c_float(0)
    inf, nan = float("inf"), float("nan")
    for tl, th in ((inf, inf), (nan, nan), (1.0, nan), (nan, 1.0), (1.0, inf)):
        assert host.ek_decide(tl, th, ctypes.addressof(k)) == 0, (tl, th)
    assert host.ek_decide(1.5, 1.5, ctypes.addressof(k)) == 1 and k.value == 1.5
    assert host.ek_decide(0.0, 0.0, ctypes.addressof(k)) == 1 and k.value == 0.0
    assert host.ek_decide(1.5, float(np.nextafter(np.float32(1.5), np.float32(2))), ctypes.addressof(k)) == 0
    dec, _ = _of(host, [inf, nan, 1e308], [0.0, 0.0, 1e308])
    assert not dec.any()


def test_every_size_is_fused_as_the_resource_table_says(host):
    """kEmbedKeyFused<b>: the sizes whose key comes out of the embed passes; the committed
    resource table lists a key variant for each of them."""
    with open(os.path.join(ROOT, "profiles", "embed_key", "resource_usage.txt")) as f:
        table = f.read()
    for b in BLOCKS:
        fused = host.ek_fused(b)
        assert fused in (0, 1)
        assert bool(re.search(r"^embed_key_kernel<%d, false>" % b, table, re.M)) == bool(fused), b
    assert host.ek_fused(5) == -1


@pytest.mark.parametrize("b", (4, 8, 10, 16))
def test_helper_prediction_on_ordinary_covers(b):
    """embed_key_helpers.predict on covers with every kind of block: a decided key is the
    oracle's dgesdd-route f32 S[0] (keyed_helpers.key_of); zero and flat blocks are uncertified
    and decided."""
    from golden.gen_golden import cover
    from keyed_helpers import key_of

    H, W = 4 * b, 12 * b
    noise = cover("noise", H, W, 3 * b)
    noise[:b, :b] = 0  # a zero block
    noise[:b, b:2 * b] = (10, 200, 30)  # a flat block
    cert, dec, key = EK.predict(noise, b)
    assert not cert[0, 0] and not cert[0, 1] and dec[0, 0] and dec[0, 1] and key[0, 0] == 0.0
    assert cert.sum() >= cert.size - 4
    ref = key_of(noise, b)
    assert np.array_equal(key[dec].view(np.uint32), ref[dec].view(np.uint32))
    assert dec.mean() > 0.95
