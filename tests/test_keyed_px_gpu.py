"""The keyed calls on 4-byte pixels on the GPU: sigma1_map / extract_keyed read
R G B pad frames where they lie and give the key bits and tile bytes of the 3-byte calls on the
same R, G, B values -- through the strip pass, the list pass and the dgesdd route, on every route,
aligned and unaligned bases and strides, host and device memory, ragged batches, the enrolment
call's four layout pairs and the drop-ins' zero-copy route."""
import ctypes
import gc
import os
import sys

import numpy as np
import pytest
from PIL import Image

from oracle import oracle as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from keyed_helpers import key_of, sparks  # noqa: E402

BLOCKS = (4, 6, 8, 10, 12, 14, 16)
ROUTES = ("hybrid", "reference", "rank1", "rank1_reference")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from thatsmyface_amd import _lib

    assert _lib.device_count() > 0
    return torch.device("cuda", 0)


def _u8(seed, shape):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def _bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _rgbx(rgb: np.ndarray, seed: int) -> np.ndarray:
    """(..., 3) -> (..., 4): the same R, G, B and random pad bytes."""
    out = _u8(seed, rgb.shape[:-1] + (4,))
    out[..., :3] = rgb
    return out


def _covers(H, W, b, seed):
    """noise, camera-like and sparks (every block strip pass -> list pass -> dgesdd route)"""
    from golden.gen_golden import cover
    from lapack_path import photo_cover

    return np.ascontiguousarray(np.stack([cover("noise", H, W, seed), photo_cover(H, W, seed + 1), sparks(H, W, b, seed + 2)]))


def _shapes(b):
    return ((3 * b + 3, 35 * b + 5), (4 * b, 64 * b))  # tests/test_keyed_gpu.py's


@pytest.mark.parametrize("b", BLOCKS)
def test_key_bits_equal_the_3_byte_call(dev, b):
    from thatsmyface_amd import batch

    for H, W in _shapes(b):
        host = _covers(H, W, b, 10 * b)
        nb = (H // b) * (W // b)
        f3 = torch.from_numpy(host).to(dev)
        f4 = torch.from_numpy(_rgbx(host, 11 * b)).to(dev)
        keys = {}
        for route in ("hybrid", "reference"):
            s3, s4 = {}, {}
            k3 = batch.sigma1_map(f3, b, stats=s3, route=route)
            k4 = batch.sigma1_map(f4, b, stats=s4, route=route)
            assert k4.dtype == torch.float32 and tuple(k4.shape) == (3, H // b, W // b)
            assert np.array_equal(_bits(k4), _bits(k3)), (H, W, route)
            assert s4 == s3, (H, W, route, s3, s4)  # the passes' decisions depend on the pixels only
            keys[route] = k4
        assert np.array_equal(_bits(keys["hybrid"]), _bits(keys["reference"]))
        for f in range(3):
            assert np.array_equal(_bits(keys["hybrid"][f]), _bits(key_of(host[f], b))), (H, W, f)
        for route in ROUTES[2:]:
            assert np.array_equal(_bits(batch.sigma1_map(f4, b, route=route)), _bits(keys["hybrid"])), route
        # sparks alone on the hybrid route: every block through the list pass to the dgesdd route
        st = {}
        batch.sigma1_map(f4[2:], b, stats=st)
        assert st == {"lapack_blocks": nb, "list_pass_blocks": nb}, (st, nb)


@pytest.mark.parametrize("b", BLOCKS)
def test_keyed_extract_equals_the_3_byte_call_and_the_oracle(dev, b):
    from golden.gen_golden import wmark

    from thatsmyface_amd import batch

    for H, W in _shapes(b):
        nbh, nbw = H // b, W // b
        covers = _covers(H, W, b, 20 * b)
        tiles = torch.from_numpy(np.stack([wmark(k, nbh, nbw, 3 + i) for i, k in enumerate(("noise", "qr", "pattern"))])).to(dev)
        for shared in (True, False):
            host = np.ascontiguousarray(np.stack([covers[0]] * 3)) if shared else covers
            fr = torch.from_numpy(host).to(dev)
            key = batch.sigma1_map(fr[:1], b)[0] if shared else batch.sigma1_map(fr, b)
            for alpha in (0.1, -0.5):
                w3 = batch.embed_batch(fr, tiles, b, alpha)
                w_h = w3.cpu().numpy()
                w4 = torch.from_numpy(_rgbx(w_h, 21 * b)).to(dev)
                ref = np.stack([O.extract_frame(w_h[f], host[f], b, alpha, route="lapack") for f in range(3)])
                for route in ROUTES:
                    s3, s4 = {}, {}
                    g3 = batch.extract_keyed(w3, key, b, alpha, route=route, stats=s3)
                    g4 = batch.extract_keyed(w4, key, b, alpha, route=route, stats=s4)
                    assert torch.equal(g4, g3), (H, W, shared, alpha, route)
                    assert np.array_equal(g4.cpu().numpy(), ref), (H, W, shared, alpha, route)
                    assert s4 == s3, (H, W, shared, alpha, route, s3, s4)
                out = torch.full((3, nbh, nbw), 7, dtype=torch.uint8, device=dev)  # asynchronous, a caller's buffer
                assert batch.extract_keyed(w4, key, b, alpha, out=out) is out
                torch.cuda.synchronize()
                assert np.array_equal(out.cpu().numpy(), ref)
        # sparks frames, watermarked: every block of the extract on the dgesdd route as well
        sp = np.ascontiguousarray(np.stack([sparks(H, W, b, 30 + f) for f in range(2)]))
        sf = torch.from_numpy(sp).to(dev)
        ws = batch.embed_batch(sf, tiles[0], b, 0.1)
        s3, s4 = {}, {}
        g3 = batch.extract_keyed(ws, batch.sigma1_map(sf, b), b, 0.1, stats=s3)
        g4 = batch.extract_keyed(torch.from_numpy(_rgbx(ws.cpu().numpy(), 31)).to(dev), batch.sigma1_map(sf, b), b, 0.1, stats=s4)
        assert torch.equal(g4, g3) and s4 == s3, (s3, s4)


def test_python_layer_keeps_refusing_4_byte_frames_elsewhere(dev):
    from thatsmyface_amd import batch

    f4 = torch.zeros((1, 16, 16, 4), dtype=torch.uint8, device=dev)
    t = torch.zeros((2, 2), dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match=r"\(N, H, W, 3\)"):
        batch.embed_batch(f4, t, 8, 0.1)
    with pytest.raises(ValueError, match=r"\(N, H, W, 3\)"):
        batch.extract_batch(f4, f4, 8, 0.1)
    with pytest.raises(ValueError, match=r"\(H, W, 3\)"):
        batch.embed_ragged([f4[0]], [t], 8, 0.1)
    with pytest.raises(ValueError, match=r"\(H, W, 3\)"):
        batch.extract_ragged([f4[0]], [f4[0]], 8, 0.1)
    with pytest.raises(ValueError, match="mixes 3- and 4-byte pixels"):
        batch.sigma1_map_ragged([f4[0], f4[0, :, :, :3].contiguous()], 8)


@pytest.mark.parametrize("b", (8, 6))
def test_layout_corners_through_the_c_entry(dev, b):
    """A base pointer 1 byte into a buffer (the byte-load path), a padded frame stride that is no
    multiple of 4 (bytes again), one that is (dwords), on device and on host memory."""
    from thatsmyface_amd import _lib, batch

    L = _lib.load()
    H, W, n = 3 * b + 3, 35 * b + 5, 3
    nbh, nbw = H // b, W // b
    host = _covers(H, W, b, 50 + b)
    f3 = torch.from_numpy(host).to(dev)
    key = batch.sigma1_map(f3, b)
    wm = batch.embed_batch(f3, torch.from_numpy(_u8(51, (nbh, nbw))).to(dev), b, 0.1)
    tiles = batch.extract_keyed(wm, key, b, 0.1)
    wm_h, key_h = wm.cpu().numpy(), key.cpu().numpy()
    fb = H * W * 4
    for offset, stride in ((1, fb), (0, fb + 7), (0, fb + 8), (0, fb)):
        for src, want_key in ((host, True), (wm_h, False)):
            buf = _u8(52, (offset + n * stride + 16,))
            for f in range(n):
                buf[offset + f * stride: offset + f * stride + fb] = _rgbx(src[f], 53 + f).reshape(-1)
            dbuf = torch.from_numpy(buf).to(dev)
            for mem, base in ((_lib.MEM_DEVICE, dbuf.data_ptr() + offset), (_lib.MEM_HOST, buf.ctypes.data + offset)):
                cnt = ctypes.c_int64(-1)
                with torch.cuda.device(dev):
                    if want_key:
                        out = torch.zeros_like(key) if mem == _lib.MEM_DEVICE else np.zeros((n, nbh, nbw), np.float32)
                        ptr = out.data_ptr() if mem == _lib.MEM_DEVICE else out.ctypes.data
                        _lib.check(L.tmfwm_sigma1_map_px(base, 4, stride, n, H, W, b, ptr, mem, None, 0, ctypes.addressof(cnt)), "map")
                        assert np.array_equal(_bits(out), _bits(key)), (offset, stride, mem)
                    else:
                        out = torch.zeros_like(tiles) if mem == _lib.MEM_DEVICE else np.zeros((n, nbh, nbw), np.uint8)
                        ptr = out.data_ptr() if mem == _lib.MEM_DEVICE else out.ctypes.data
                        _lib.check(L.tmfwm_extract_keyed_px(base, 4, stride, n, H, W, key.data_ptr() if mem == _lib.MEM_DEVICE
                                                            else key_h.ctypes.data, nbh * nbw * 4, b, 0.1, ptr, mem, None, 0,
                                                            ctypes.addressof(cnt)), "keyed")
                        got = out.cpu().numpy() if mem == _lib.MEM_DEVICE else out
                        assert np.array_equal(got, tiles.cpu().numpy()), (offset, stride, mem)
                assert cnt.value >= nbh * nbw  # the sparks frame's blocks at least
    # pixel_bytes == 3 through the same entry is the sibling
    out = torch.zeros_like(key)
    with torch.cuda.device(dev):
        _lib.check(L.tmfwm_sigma1_map_px(f3.data_ptr(), 3, H * W * 3, n, H, W, b, out.data_ptr(), _lib.MEM_DEVICE, None, 0, None), "map")
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out), _bits(key))
    with torch.cuda.device(dev):  # an overlapping output is refused at either pixel size
        with pytest.raises(ValueError, match="overlaps"):
            _lib.check(L.tmfwm_sigma1_map_px(dbuf.data_ptr(), 4, fb, n, H, W, b, dbuf.data_ptr() + 16, _lib.MEM_DEVICE, None, 0, None), "map")


@pytest.mark.parametrize("b", (4, 8, 14))
def test_ragged_frames_of_mixed_sizes(dev, b):
    from thatsmyface_amd import _lib, batch

    sizes = [(3 * b + 3, 35 * b + 5), (b - 1, 5 * b), (2 * b, 9 * b + 1), (b, b), (4 * b + 2, 70 * b)]
    # noise, (too small for a block), sparks, one block of noise, camera-like
    hosts = [_covers(H, W, b, 60 + i)[i % 3] if H >= 2 * b else _u8(60 + i, (H, W, 3)) for i, (H, W) in enumerate(sizes)]
    f3 = [torch.from_numpy(h).to(dev) for h in hosts]
    f4 = [torch.from_numpy(_rgbx(h, 70 + i)).to(dev) for i, h in enumerate(hosts)]
    for route in ("hybrid", "reference"):
        s3, s4 = {}, {}
        k3 = batch.sigma1_map_ragged(f3, b, stats=s3, route=route)
        k4 = batch.sigma1_map_ragged(f4, b, stats=s4, route=route)
        assert s3 == s4, (route, s3, s4)
        for i, (a, c) in enumerate(zip(k3, k4)):
            assert tuple(c.shape) == (sizes[i][0] // b, sizes[i][1] // b)
            assert np.array_equal(_bits(a), _bits(c)), (route, i)
            if c.numel():
                assert np.array_equal(_bits(c), _bits(batch.sigma1_map(f4[i][None], b)[0])), (route, i)
    keys = batch.sigma1_map_ragged(f4, b)
    tiles = [torch.from_numpy(_u8(80 + i, (H // b, W // b))).to(dev) for i, (H, W) in enumerate(sizes)]
    w3 = batch.embed_ragged(f3, tiles, b, 0.1)
    w4 = [torch.from_numpy(_rgbx(w.cpu().numpy(), 90 + i)).to(dev) for i, w in enumerate(w3)]
    for route in ("hybrid", "reference"):
        s3, s4 = {}, {}
        g3 = batch.extract_keyed_ragged(w3, keys, b, 0.1, stats=s3, route=route)
        g4 = batch.extract_keyed_ragged(w4, keys, b, 0.1, stats=s4, route=route)
        assert s3 == s4, (route, s3, s4)
        for i, (a, c) in enumerate(zip(g3, g4)):
            assert torch.equal(a, c), (route, i)
            if c.numel():
                assert torch.equal(c, batch.extract_keyed(w4[i][None], keys[i], b, 0.1)[0]), (route, i)
                assert np.array_equal(c.cpu().numpy(), O.extract_frame(w3[i].cpu().numpy(), hosts[i], b, 0.1, route="lapack")), (route, i)
    # many frames pointing at one key
    many = [w4[0], torch.from_numpy(_rgbx(hosts[0], 99)).to(dev), w4[0]]
    got = batch.extract_keyed_ragged(many, [keys[0]] * 3, b, 0.1)
    assert torch.equal(got[0], g4[0]) and torch.equal(got[2], g4[0])
    assert torch.equal(got[1], batch.extract_keyed(f3[0][None], keys[0], b, 0.1)[0])
    # host memory through the C entry: a frame without a block keeps its output, one of zero width is skipped
    L = _lib.load()
    hw = [w.cpu().numpy() for w in w4] + [np.zeros((b, 0, 4), np.uint8)]
    hk = [k.cpu().numpy() for k in keys] + [np.zeros((1, 0), np.float32)]
    ko = [np.full(k.shape, -7.0, np.float32) for k in hk]
    to = [np.full(k.shape, 7, np.uint8) for k in hk]
    h4 = [f.cpu().numpy() for f in f4] + [np.zeros((b, 0, 4), np.uint8)]
    md = (_lib.KeyFrame * len(hw))(*[_lib.KeyFrame(f.ctypes.data, o.ctypes.data, f.shape[0], f.shape[1]) for f, o in zip(h4, ko)])
    kd = (_lib.KeyedFrame * len(hw))(*[_lib.KeyedFrame(f.ctypes.data, k.ctypes.data, o.ctypes.data, f.shape[0], f.shape[1])
                                       for f, k, o in zip(hw, hk, to)])
    md[5].rgb, md[5].out_key, kd[5].wm_rgb, kd[5].key, kd[5].out_tile = None, None, None, None, None  # not looked at
    md[1].out_key, kd[1].key, kd[1].out_tile = None, None, None  # height < block: no block, nothing written
    with torch.cuda.device(dev):
        _lib.check(L.tmfwm_sigma1_map_ragged_px(ctypes.addressof(md), len(hw), b, 4, _lib.MEM_HOST, None, 0, None), "map")
        _lib.check(L.tmfwm_extract_keyed_ragged_px(ctypes.addressof(kd), len(hw), b, 0.1, 4, _lib.MEM_HOST, None, 0, None), "keyed")
    for i in range(5):
        assert np.array_equal(_bits(ko[i]), _bits(keys[i])), i
        assert np.array_equal(to[i], g4[i].cpu().numpy()), i


@pytest.mark.parametrize("b", (8, 12))
def test_embed_with_key_layout_pairs(dev, b):
    from thatsmyface_amd import batch

    H, W = 3 * b + 3, 35 * b + 5
    host = _covers(H, W, b, 100 + b)
    f3 = torch.from_numpy(host).to(dev)
    f4 = torch.from_numpy(_rgbx(host, 101)).to(dev)
    tile = torch.from_numpy(_u8(102, (3, H // b, W // b))).to(dev)
    key = batch.sigma1_map(f3, b)
    for route in ROUTES:
        ref = batch.embed_batch(f3, tile, b, 0.1, route=route)
        for src in (f3, f4):
            for opx in (3, 4):
                out = torch.full((3, H, W, opx), 9, dtype=torch.uint8, device=dev)
                got, k = batch.embed_with_key(src, tile, b, 0.1, out=out, route=route, stats={})
                assert got is out
                assert torch.equal(got[..., :3], ref), (route, src.shape[-1], opx)
                if opx == 4:
                    assert bool((got[..., 3] == 255).all()), (route, src.shape[-1])
                assert np.array_equal(_bits(k), _bits(key)), (route, src.shape[-1], opx)
        got, k = batch.embed_with_key(f4, tile, b, 0.1, route=route)  # 4-byte frames give 4-byte output
        torch.cuda.synchronize()
        assert tuple(got.shape) == (3, H, W, 4) and torch.equal(got[..., :3], ref) and bool((got[..., 3] == 255).all())
        assert np.array_equal(_bits(k), _bits(key))


def test_embed_key_px_host_memory_and_padded_key_stride(dev):
    from thatsmyface_amd import _lib, batch

    L = _lib.load()
    b, H, W, n = 8, 27, 45, 2
    nbh, nbw = H // b, W // b
    host = _u8(110, (n, H, W, 3))
    h4 = _rgbx(host, 111)
    tile = _u8(112, (nbh, nbw))
    f3 = torch.from_numpy(host).to(dev)
    ref = batch.embed_batch(f3, torch.from_numpy(tile).to(dev), b, 0.1).cpu().numpy()
    key = batch.sigma1_map(f3, b).cpu().numpy()
    out = np.zeros((n, H, W, 4), np.uint8)
    kout = np.full((n, nbh * nbw + 3), np.nan, np.float32)
    with torch.cuda.device(dev):
        _lib.check(L.tmfwm_embed_key_px(h4.ctypes.data, 4, H * W * 4, n, H, W, tile.ctypes.data, 0, b, 0.1, out.ctypes.data, 4,
                                        H * W * 4, kout.ctypes.data, (nbh * nbw + 3) * 4, _lib.MEM_HOST, None, 0, None), "embed_key_px")
    assert np.array_equal(out[..., :3], ref) and (out[..., 3] == 255).all()
    assert np.array_equal(_bits(kout[:, : nbh * nbw].reshape(n, nbh, nbw)), _bits(key))
    assert np.isnan(kout[:, nbh * nbw:]).all()  # the padding is not written


def test_dropins_take_the_zero_copy_route(dev, monkeypatch):
    from thatsmyface_amd import watermarking as Wm

    pa = Wm._arrow()
    assert pa is not None, "the zero-copy route needs pyarrow and Pillow's Arrow interface"
    cfg = {"block_size": 8, "alpha": 0.1}
    wm = Image.fromarray(_u8(120, (40, 40)), "L")
    calls = []
    real = Wm._rgbx_view

    def spy(image):
        v = real(image)
        calls.append(v is not None)
        return v

    monkeypatch.setattr(Wm, "_rgbx_view", spy)
    for h, w in ((96, 160), (1080, 1920)):
        rgb = _u8(121, (h, w, 3))
        cover = Image.fromarray(rgb)
        monkeypatch.setattr(Wm, "_zero_copy", False)
        key0 = Wm.extraction_key(cover, cfg)
        img0, ekey0 = Wm.embed_watermark_with_key(cover, wm, False, cfg)
        ext0 = np.asarray(Wm.extract_watermark_keyed(img0, key0, cfg))
        assert not calls and not hasattr(img0, "_tmfwm_rgbx")
        monkeypatch.setattr(Wm, "_zero_copy", True)
        key1 = Wm.extraction_key(cover, cfg)
        img1, ekey1 = Wm.embed_watermark_with_key(cover, wm, False, cfg)
        assert calls == [True, True], calls  # PIL's own pixels went to the library both times
        assert img1.mode == "RGB" and img1.size == cover.size and hasattr(img1, "_tmfwm_rgbx")
        assert np.array_equal(_bits(key1), _bits(key0)) and np.array_equal(_bits(ekey1), _bits(key0))
        assert np.array_equal(_bits(ekey0), _bits(key0))
        assert np.array_equal(np.asarray(img1), np.asarray(img0))
        assert np.array_equal(np.asarray(img1), np.asarray(Wm.embed_watermark(cover, wm, False, cfg)))
        ext1 = np.asarray(Wm.extract_watermark_keyed(img1, key1, cfg))  # the embed's own buffer, read back in place
        ext2 = np.asarray(Wm.extract_watermark_keyed(Image.fromarray(np.asarray(img1)), key1, cfg))  # a fresh PIL image
        assert calls[-2:] == [True, True]
        assert np.array_equal(ext1, ext0) and np.array_equal(ext2, ext0)
        assert np.array_equal(ext0, np.asarray(Wm.extract_watermark(img0, cover, cfg)))
        # a read-only image takes the copying path and gives the same results
        x = _rgbx(rgb, 123).reshape(-1)  # an Arrow-backed image that is not one of the drop-in's own
        vals = pa.Array.from_buffers(pa.uint8(), w * h * 4, [None, pa.py_buffer(x)])
        ro = Image.fromarrow(pa.FixedSizeListArray.from_arrays(vals, 4), "RGB", (w, h))
        assert ro.readonly and np.array_equal(np.asarray(ro), rgb)
        del calls[:]
        assert np.array_equal(_bits(Wm.extraction_key(ro, cfg)), _bits(key0))
        imgr, keyr = Wm.embed_watermark_with_key(ro, wm, False, cfg)
        assert calls == [False, False], calls
        assert np.array_equal(np.asarray(imgr), np.asarray(img0)) and np.array_equal(_bits(keyr), _bits(key0))
        # an in-place edit makes PIL copy the pixels first: the keyed extract must see the edit,
        # and the pool's buffer must not
        kept = img1._tmfwm_rgbx.copy()
        img1.paste((255, 0, 0), (0, 0, 64, 64))
        edited = np.asarray(img1)
        assert np.array_equal(img1._tmfwm_rgbx, kept)
        monkeypatch.setattr(Wm, "_zero_copy", False)
        want = np.asarray(Wm.extract_watermark_keyed(Image.fromarray(edited), key0, cfg))
        monkeypatch.setattr(Wm, "_zero_copy", True)
        assert np.array_equal(np.asarray(Wm.extract_watermark_keyed(img1, key0, cfg)), want)
        del calls[:]
    # pool: a live output keeps its buffer; a dropped one gives it back
    cover = Image.fromarray(_u8(122, (64, 96, 3)))
    a, _ = Wm.embed_watermark_with_key(cover, wm, False, cfg)
    b2, _ = Wm.embed_watermark_with_key(cover, wm, False, cfg)
    assert a._tmfwm_rgbx is not b2._tmfwm_rgbx
    buf = b2._tmfwm_rgbx.ctypes.data
    del b2
    gc.collect()
    c, _ = Wm.embed_watermark_with_key(cover, wm, False, cfg)
    assert c._tmfwm_rgbx.ctypes.data == buf and np.array_equal(np.asarray(c), np.asarray(a))
