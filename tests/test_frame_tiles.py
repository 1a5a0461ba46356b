"""One watermark tile per frame (tmfwm_embed_tiles, tmfwm_embed_multi_tiles, tmfwm_prepare_tiles,
a sequence of watermarks in pipeline.embed_images): what can be checked without a GPU --
argument checks that run before any device work, the shapes the Python layer accepts, and the
pipeline's order with the oracle standing in for the device stage.  The GPU side is
tests/test_frame_tiles_gpu.py.
"""
import io

import numpy as np
import pytest
from PIL import Image

from oracle import oracle as O
from thatsmyface_amd import _lib, multi, pipeline


def test_argument_validation_before_device():
    L = _lib.load()
    p = lambda x: x.ctypes.data  # noqa: E731
    n, H, W, b = 3, 16, 24, 8
    tb = (H // b) * (W // b)  # 6 bytes per tile
    a = np.zeros((n, H, W, 3), np.uint8)
    a4 = np.zeros((n, H, W, 4), np.uint8)
    o, o4 = np.empty_like(a), np.empty_like(a4)
    t = np.zeros((n, tb + 8), np.uint8)
    f3, f4 = H * W * 3, H * W * 4

    def tiles(ipx=3, istride=f3, stride=tb, block=b, opx=3, ostride=f3, route=0, src=a, dst=o):
        _lib.check(L.tmfwm_embed_tiles(p(src), ipx, istride, n, H, W, p(t), stride, block, 0.1, p(dst), opx, ostride, _lib.MEM_HOST,
                                       None, route, None), "embed_tiles")

    # a stride that is neither 0 (one shared tile) nor at least a tile, in both layouts' code paths
    for bad in (1, tb - 1, -1, -tb):
        with pytest.raises(ValueError, match="tile_stride"):
            tiles(stride=bad)
        with pytest.raises(ValueError, match="tile_stride"):
            tiles(ipx=4, istride=f4, stride=bad, opx=4, ostride=f4, src=a4, dst=o4)
    for px in (2, 5):
        with pytest.raises(ValueError, match="pixel bytes"):
            tiles(ipx=px, istride=f4, opx=4, ostride=f4, src=a4, dst=o4)
        with pytest.raises(ValueError, match="pixel bytes"):
            tiles(ipx=4, istride=f4, opx=px, ostride=f4, src=a4, dst=o4)
    with pytest.raises(ValueError, match="one frame_stride"):
        tiles(ostride=f3 + 4)
    for kw in ({}, dict(ipx=4, istride=f4, opx=4, ostride=f4, src=a4, dst=o4)):
        with pytest.raises(NotImplementedError):
            tiles(block=7, **kw)
        with pytest.raises(ValueError, match="route"):
            tiles(route=4, **kw)
    with pytest.raises(ValueError, match="tile_stride"):
        _lib.check(L.tmfwm_embed_multi_tiles(p(a), n, H, W, f3, p(t), tb - 1, b, 0.1, p(o), None, 0, 0, None), "embed_multi_tiles")

    # tmfwm_prepare_tiles: sizes and strides
    wm = np.zeros((n, 29 * 29 + 3), np.uint8)
    out = np.zeros((n, 17 * 25 + 5), np.uint8)

    def prep(h=29, w=29, ws=29 * 29 + 3, th=17, tw=25, ts=17 * 25 + 5, count=n):
        _lib.check(L.tmfwm_prepare_tiles(p(wm), count, h, w, ws, th, tw, 1, p(out), ts, _lib.MEM_HOST, None), "prepare_tiles")

    for kw in (dict(h=0), dict(w=-1), dict(th=0), dict(tw=0), dict(count=-1)):
        with pytest.raises(ValueError):
            prep(**kw)
    with pytest.raises(ValueError, match="wm_stride"):
        prep(ws=29 * 29 - 1)
    with pytest.raises(ValueError, match="tile_stride"):
        prep(ts=17 * 25 - 1)

    # multi.embed_multi: a 3-D tile has one (H/b, W/b) tile per frame
    for shape in ((n + 1, H // b, W // b), (n, H // b + 1, W // b), (n, 1, H // b, W // b), (tb,)):
        with pytest.raises(ValueError, match="wm_tile"):
            multi.embed_multi(a, np.zeros(shape, np.uint8), b, 0.1)


@pytest.mark.skipif(_lib.device_count() > 0, reason="CPU-only check")
def test_per_frame_tiles_accepted_without_device():
    """The API takes an (N, H/b, W/b) tile: what fails on a box without a GPU is the device, not the shape."""
    a = np.zeros((3, 16, 24, 3), np.uint8)
    with pytest.raises(_lib.TmfwmError, match="no HIP device"):
        multi.embed_multi(a, np.zeros((3, 2, 3), np.uint8), 8, 0.1)
    L = _lib.load()
    t, o = np.zeros((3, 6), np.uint8), np.empty_like(a)
    with pytest.raises(_lib.TmfwmError, match="no HIP device"):
        _lib.check(L.tmfwm_embed_tiles(a.ctypes.data, 3, a[0].size, 3, 16, 24, t.ctypes.data, 6, 8, 0.1, o.ctypes.data, 3, a[0].size,
                                       _lib.MEM_HOST, None, 0, None), "embed_tiles")
    w = np.zeros((3, 29, 29), np.uint8)
    with pytest.raises(_lib.TmfwmError, match="no HIP device"):
        _lib.check(L.tmfwm_prepare_tiles(w.ctypes.data, 3, 29, 29, 29 * 29, 2, 3, 1, t.ctypes.data, 6, _lib.MEM_HOST, None), "prepare_tiles")


def _images(n, seed=0):
    from lapack_path import photo_cover

    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        h, w = [(96, 128), (120, 90), (96, 128), (64, 200)][i % 4]
        arr = photo_cover(h, w, seed + i) if i % 2 else rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        buf = io.BytesIO()
        Image.fromarray(arr).save(buf, format="PNG")
        out.append(buf.getvalue() if i % 3 else Image.fromarray(arr))
    return out


def _wm(seed):
    return Image.fromarray((np.random.default_rng(seed).integers(0, 2, (29, 29)) * 255).astype(np.uint8), "L")


def _wm_png(seed):
    buf = io.BytesIO()
    _wm(seed).save(buf, format="PNG")
    return buf.getvalue()


def _oracle_stage(greys, block, alpha, preserve_ratio, calls):
    def stage(rgb, i):
        calls.append(i)
        tile = O.prepare_tile(greys[i], rgb.shape[0] // block, rgb.shape[1] // block, preserve_ratio)
        return O.embed_frame(rgb, tile, block, alpha), None

    return stage


def test_pipeline_watermark_per_image_cpu():
    """embed_images with a sequence of watermarks: image i gets watermark i (PNG bytes or PIL
    image), in order, pixels and PNG equal to the per-image oracle result."""
    n = 7
    imgs = _images(n)
    wms = [_wm_png(100 + i) if i % 2 else _wm(100 + i) for i in range(n)]
    greys = [np.asarray(_wm(100 + i)) for i in range(n)]
    assert len({g.tobytes() for g in greys}) == n
    for seq in (list, tuple):
        calls = []
        res = pipeline.embed_images(imgs, seq(wms), True, {"block_size": 8, "alpha": 0.1}, workers=4,
                                    device_stage=_oracle_stage(greys, 8, 0.1, True, calls))
        assert calls == list(range(n)) and len(res) == n
        for i, (src, r) in enumerate(zip(imgs, res)):
            rgb = pipeline._decode(src)
            ref = O.embed_frame(rgb, O.prepare_tile(greys[i], rgb.shape[0] // 8, rgb.shape[1] // 8, True), 8, 0.1)
            assert np.array_equal(r.pixels, ref), i
            assert np.array_equal(np.asarray(Image.open(io.BytesIO(r.png))), ref), i
    # images 0 and 2 have one size but different watermarks: the result depends on the watermark
    a, b = pipeline._decode(imgs[0]), pipeline._decode(imgs[2])
    assert a.shape == b.shape
    same_cover = pipeline.embed_images([imgs[0], imgs[0]], wms[:2], True, {"block_size": 8, "alpha": 0.1}, workers=2,
                                       device_stage=_oracle_stage(greys, 8, 0.1, True, []))
    assert not np.array_equal(same_cover[0].pixels, same_cover[1].pixels)
    for bad in (wms[:-1], wms + [wms[0]], []):
        with pytest.raises(ValueError, match="watermarks"):
            pipeline.embed_images(imgs, bad, True, {"block_size": 8, "alpha": 0.1}, device_stage=_oracle_stage(greys, 8, 0.1, True, []))
    # a single watermark still calls stage(rgb)
    single = pipeline.embed_images(imgs[:2], wms[1], True, {"block_size": 8, "alpha": 0.1}, workers=2,
                                   device_stage=lambda rgb: (O.embed_frame(rgb, O.prepare_tile(greys[1], rgb.shape[0] // 8,
                                                                                               rgb.shape[1] // 8, True), 8, 0.1), None))
    assert len(single) == 2
