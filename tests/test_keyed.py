"""Keyed extraction on the CPU: the new entry points exist and agree across the
header, the library and the ctypes table; they validate their arguments before any device
work; the drop-in functions check the key; and the expected-value builder the GPU tests
compare against (keyed_helpers) reproduces the oracle's extract from two keys, byte for byte."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

from oracle import oracle as O
from thatsmyface_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from keyed_helpers import bytes_of, key_of, sparks  # noqa: E402

NAMES = ("tmfwm_sigma1_map", "tmfwm_extract_keyed")
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
    assert len(_lib.SIGNATURES["tmfwm_sigma1_map"][1]) == 11 and len(_lib.SIGNATURES["tmfwm_extract_keyed"][1]) == 14
    assert L.tmfwm_abi_version() == 10  # added within ABI 10


def test_argument_validation_before_device():
    L = _lib.load()
    a = np.zeros((16, 16, 3), np.uint8)
    k = np.zeros((2, 2), np.float32)
    t = np.zeros((2, 2), np.uint8)
    H = _lib.MEM_HOST

    def smap(n=1, block=8, route=0):
        return L.tmfwm_sigma1_map(_p(a), n, 16, 16, a.size, block, _p(k), H, None, route, None)

    def xkey(n=1, block=8, route=0, alpha=0.1, stride=0):
        return L.tmfwm_extract_keyed(_p(a), n, 16, 16, a.size, _p(k), stride, block, alpha, _p(t), H, None, route, None)

    for bad_block in (7, 18, 2):
        with pytest.raises(NotImplementedError):
            _lib.check(smap(block=bad_block), "sigma1_map")
        with pytest.raises(NotImplementedError):
            _lib.check(xkey(block=bad_block), "extract_keyed")
    for bad_route in (-1, 4):
        with pytest.raises(ValueError, match="route"):
            _lib.check(smap(route=bad_route), "sigma1_map")
        with pytest.raises(ValueError, match="route"):
            _lib.check(xkey(route=bad_route), "extract_keyed")
    for bad_alpha in (0.0, float("nan")):
        with pytest.raises(ValueError, match="alpha"):
            _lib.check(xkey(alpha=bad_alpha), "extract_keyed")
    nbh = nbw = 2
    for bad_stride in (2, nbh * nbw * 4 - 4, -16):
        with pytest.raises(ValueError, match="key_stride"):
            _lib.check(xkey(n=1, stride=bad_stride), "extract_keyed")
    with pytest.raises(ValueError, match="negative"):
        _lib.check(smap(n=-1), "sigma1_map")
    with pytest.raises(ValueError, match="negative"):
        _lib.check(xkey(n=-1), "extract_keyed")
    with pytest.raises(ValueError, match="frame_stride"):
        _lib.check(L.tmfwm_sigma1_map(_p(a), 2, 16, 16, 10, 8, _p(k), H, None, 0, None), "sigma1_map")


@pytest.mark.skipif(_lib.device_count() > 0, reason="CPU-only check")
def test_fails_loudly_without_gpu():
    from thatsmyface_amd import watermarking as W

    L = _lib.load()
    a = np.zeros((16, 16, 3), np.uint8)
    k = np.zeros((2, 2), np.float32)
    t = np.zeros((2, 2), np.uint8)
    with pytest.raises(_lib.TmfwmError, match="no HIP device"):
        _lib.check(L.tmfwm_sigma1_map(_p(a), 1, 16, 16, a.size, 8, _p(k), _lib.MEM_HOST, None, 0, None), "sigma1_map")
    with pytest.raises(_lib.TmfwmError, match="no HIP device"):
        _lib.check(L.tmfwm_extract_keyed(_p(a), 1, 16, 16, a.size, _p(k), 0, 8, 0.1, _p(t), _lib.MEM_HOST, None, 0, None), "x")
    s = {"block_size": 8, "alpha": 0.1}
    with pytest.raises(_lib.TmfwmError, match="no HIP device"):
        W.extraction_key(Image.new("RGB", (16, 16)), s)
    with pytest.raises(_lib.TmfwmError, match="no HIP device"):
        W.extract_watermark_keyed(Image.new("RGB", (16, 16)), k, s)


def test_dropin_key_checks_and_tiny_images():
    from thatsmyface_amd import watermarking as W
    from thatsmyface_amd.modules import watermarking as M

    assert M.extraction_key is W.extraction_key and M.extract_watermark_keyed is W.extract_watermark_keyed
    s = {"block_size": 8, "alpha": 0.1}
    img = Image.new("RGB", (32, 24))  # 3 x 4 blocks
    for bad in (np.zeros((3, 4), np.float64), np.zeros((3, 4), np.uint8), [[0.0] * 4] * 3, None):
        with pytest.raises(TypeError, match="float32"):
            W.extract_watermark_keyed(img, bad, s)
    # a key made at another block size or for another image size
    for shape in ((4, 3), (6, 8), (2, 4), (12,), (1, 3, 4)):
        with pytest.raises(ValueError, match="one block size and one image size"):
            W.extract_watermark_keyed(img, np.zeros(shape, np.float32), s)
    with pytest.raises(ValueError, match="positive"):
        W.extraction_key(img, {"block_size": 0, "alpha": 0.1})
    # an image smaller than a block: an empty key and an empty result, no device work
    for size, shape in (((5, 20), (2, 0)), ((20, 5), (0, 2)), ((3, 3), (0, 0))):
        tiny = Image.new("RGB", size)
        key = W.extraction_key(tiny, s)
        assert key.dtype == np.float32 and key.shape == shape
        ex = W.extract_watermark_keyed(tiny, key, s)
        ref = Image.fromarray(np.zeros(shape, np.uint8))
        assert ex.mode == "L" and ex.size == ref.size


def _covers(H, W, seed):
    from golden.gen_golden import cover
    from lapack_path import photo_cover

    return {"noise": cover("noise", H, W, seed), "photo": photo_cover(H, W, seed), "qr": cover("qr", H, W, seed),
            "smooth": cover("smooth", H, W, seed), "black": cover("black", H, W, seed)}


@pytest.mark.parametrize("b", BLOCKS)
def test_bytes_from_two_keys_equal_the_oracle_extract(b):
    """The argument of DESIGN.md 5 on the CPU: the original enters extract through f32(sigma_1)
    per block only, so the bytes from two keys equal the oracle's extract -- on its dgesdd route
    and on its default (hybrid) route -- with 0 differences."""
    from golden.gen_golden import wmark

    H, W = 5 * b + 3, 9 * b + 5
    for i, (kind, c) in enumerate(_covers(H, W, 100 + b).items()):
        c = np.ascontiguousarray(c)
        t = wmark("noise", H // b, W // b, 7 + i)
        for alpha in (0.1, 1.0, -0.5):
            w = O.embed_frame(c, t, b, alpha, route="lapack")
            got = bytes_of(key_of(w, b), key_of(c, b), alpha)
            assert np.array_equal(got, O.extract_frame(w, c, b, alpha, route="lapack")), (kind, alpha)
            assert np.array_equal(got, O.extract_frame(w, c, b, alpha)), (kind, alpha)


@pytest.mark.parametrize("b", BLOCKS)
def test_sparks_blocks_never_certify(b):
    """The cover the GPU tests use to force the dgesdd route: in every block of it, and of its
    watermarked version, 2 sigma_1^2 <= |D|_F^2 (all singular values nearly equal), so the
    enclosure's condition 2 rho > F cannot hold for any vector (rho <= sigma_1^2)."""
    from golden.gen_golden import wmark

    H, W = 3 * b + 3, 35 * b + 5
    c = sparks(H, W, b, 5)
    w = O.embed_frame(c, wmark("noise", H // b, W // b, 3), b, 0.1, route="lapack")
    for img in (c, w):
        y = O.rgb_to_ycbcr(img)[..., 0]
        nbh, nbw = H // b, W // b
        blocks = y[: nbh * b, : nbw * b].reshape(nbh, b, nbw, b).transpose(0, 2, 1, 3).reshape(-1, b, b)
        D = O.dct2d_blocks(np.ascontiguousarray(blocks)).astype(np.float64)
        s1 = np.linalg.svd(D, compute_uv=False)[:, 0]
        F = (D * D).sum(axis=(1, 2))
        assert (2.0 * s1 * s1 <= F).all()
