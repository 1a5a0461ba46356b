"""Ragged batches on the CPU: the two entry points are exported and declared, their arguments
are checked before any device call, a valid call without a GPU fails with TMFWM_ERR_NODEVICE,
and pipeline.embed_images groups images for a batched device stage.  No compute runs here."""
import ctypes
import io

import numpy as np
import pytest
from PIL import Image

from thatsmyface_amd import _lib, pipeline


def test_symbols_exported_and_declared():
    L = _lib.load()
    for name in ("tmfwm_embed_ragged", "tmfwm_extract_ragged"):
        assert hasattr(L, name), name
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == 8
    assert L.tmfwm_abi_version() == _lib.ABI_VERSION == 10
    # the descriptors' layout: three pointers, two int32
    assert ctypes.sizeof(_lib.EmbedFrame) == ctypes.sizeof(_lib.ExtractFrame) == 32
    assert [f[0] for f in _lib.EmbedFrame._fields_] == ["rgb", "out", "wm_tile", "height", "width"]
    assert [f[0] for f in _lib.ExtractFrame._fields_] == ["wm_rgb", "orig_rgb", "out_tile", "height", "width"]


def _calls():
    """(embed, extract): callables (block, alpha, mem_kind, route, n=None, frames=...) -> status over valid 16 x 16 descriptors."""
    L = _lib.load()
    a = np.zeros((16, 16, 3), np.uint8)
    o = np.empty_like(a)
    t = np.zeros((2, 2), np.uint8)
    keep = (a, o, t)
    ed = (_lib.EmbedFrame * 2)(_lib.EmbedFrame(a.ctypes.data, o.ctypes.data, t.ctypes.data, 16, 16),
                               _lib.EmbedFrame(a.ctypes.data, o.ctypes.data, t.ctypes.data, 16, 16))
    xd = (_lib.ExtractFrame * 2)(_lib.ExtractFrame(a.ctypes.data, a.ctypes.data, t.ctypes.data, 16, 16),
                                 _lib.ExtractFrame(a.ctypes.data, a.ctypes.data, t.ctypes.data, 16, 16))

    def embed(block=8, alpha=0.1, mem=_lib.MEM_HOST, route=0, n=2, desc=ed, _k=keep):
        return L.tmfwm_embed_ragged(ctypes.addressof(desc) if desc is not None else None, n, block, alpha, mem, None, route, None)

    def extract(block=8, alpha=0.1, mem=_lib.MEM_HOST, route=0, n=2, desc=xd, _k=keep):
        return L.tmfwm_extract_ragged(ctypes.addressof(desc) if desc is not None else None, n, block, alpha, mem, None, route, None)

    return embed, extract, ed, xd


def test_argument_validation_before_device():
    embed, extract, ed, xd = _calls()
    for call in (embed, extract):
        assert call(n=2, desc=None) == _lib.ERR_INVALID and "NULL" in _lib.last_error()  # NULL array with n > 0
        assert call(n=-1) == _lib.ERR_INVALID  # negative count
        for bad_block in (7, 18, 2):
            assert call(block=bad_block) == _lib.ERR_UNSUPPORTED
        for bad_route in (-1, 4):
            assert call(route=bad_route) == _lib.ERR_INVALID and "route" in _lib.last_error()
        for rank1 in (_lib.ROUTE_RANK1, _lib.ROUTE_RANK1_REFERENCE):
            assert call(route=rank1) == _lib.ERR_UNSUPPORTED and "rank-1" in _lib.last_error()
        for bad_mem in (-1, 2):
            assert call(mem=bad_mem) == _lib.ERR_INVALID and "mem_kind" in _lib.last_error()
        assert call(alpha=float("nan")) == _lib.ERR_INVALID and "alpha" in _lib.last_error()
    assert extract(alpha=0.0) == _lib.ERR_INVALID and "alpha" in _lib.last_error()  # divides by zero (watermarking.py:285)
    # inside a descriptor: negative sizes and NULL pointers, in the second frame, for both memory kinds
    for mem in (_lib.MEM_HOST, _lib.MEM_DEVICE):
        for field in ("height", "width"):
            for desc, call in ((ed, embed), (xd, extract)):
                old = getattr(desc[1], field)
                setattr(desc[1], field, -3)
                assert call(mem=mem) == _lib.ERR_INVALID and "frame 1" in _lib.last_error(), (mem, field)
                setattr(desc[1], field, old)
        for desc, call, fields in ((ed, embed, ("rgb", "out", "wm_tile")), (xd, extract, ("wm_rgb", "orig_rgb", "out_tile"))):
            for field in fields:
                old = getattr(desc[1], field)
                setattr(desc[1], field, None)
                assert call(mem=mem) == _lib.ERR_INVALID and "NULL" in _lib.last_error(), (mem, field)
                setattr(desc[1], field, old)
    # a frame without a block needs no tile; one of zero height needs no pointer at all (as check_frames)
    ed[1].wm_tile, ed[1].height = None, 7
    rc = embed()
    assert rc in (0, _lib.ERR_NODEVICE), _lib.last_error()
    ed[1].rgb, ed[1].out, ed[1].height = None, None, 0
    rc = embed()
    assert rc in (0, _lib.ERR_NODEVICE), _lib.last_error()
    # through the Python layer: the rank-1 routes are refused before any tensor is looked at
    batch = pytest.importorskip("thatsmyface_amd.batch")
    for route in ("rank1", "rank1_reference"):
        with pytest.raises(NotImplementedError, match="rank-1"):
            batch.embed_ragged([], [], 8, 0.1, route=route)
        with pytest.raises(NotImplementedError, match="rank-1"):
            batch.extract_ragged([], [], 8, 0.1, route=route)
    with pytest.raises(NotImplementedError):
        batch.embed_ragged([], [], 7, 0.1)


def test_valid_call_needs_a_device():
    """Without a GPU a valid call fails with TMFWM_ERR_NODEVICE (no CPU fallback); with one it runs."""
    embed, extract, _, _ = _calls()
    if _lib.device_count() > 0:
        assert embed() == 0 and extract() == 0, _lib.last_error()
        return
    for call in (embed, extract):
        for mem in (_lib.MEM_HOST, _lib.MEM_DEVICE):
            assert call(mem=mem) == _lib.ERR_NODEVICE and "no HIP device" in _lib.last_error()
        assert call(n=0, desc=None) == _lib.ERR_NODEVICE  # as tmfwm_embed with no frames


# ---- pipeline grouping with a fake batched device stage

def _images(sizes, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for i, (h, w) in enumerate(sizes):
        arr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        buf = io.BytesIO()
        Image.fromarray(arr).save(buf, format="PNG")
        out.append(buf.getvalue() if i % 2 else Image.fromarray(arr))
    return out


def _wm(i):
    return Image.fromarray(np.full((5, 5), 10 * i + 3, np.uint8), "L")


class FakeBatchedStage:
    """Marks each image with the position it was given: pixel [0, 0] = (index, group number, place in the group)."""

    def __init__(self):
        self.groups = []

    def __call__(self, rgbs, indices):
        assert len(rgbs) == len(indices)
        g = len(self.groups)
        self.groups.append(list(indices))
        out = []
        for k, (rgb, i) in enumerate(zip(rgbs, indices)):
            px = rgb.copy()
            px[0, 0] = (i, g, k)
            out.append((px, None))
        return out


SIZES = [(16, 24), (9, 40), (16, 24), (33, 17), (8, 8), (20, 20), (12, 31)]


@pytest.mark.parametrize("k,groups", [(3, [[0, 1, 2], [3, 4, 5], [6]]), (1, [[i] for i in range(7)]), (7, [list(range(7))]),
                                      (50, [list(range(7))])])
def test_pipeline_groups_in_order(k, groups):
    imgs = _images(SIZES)
    stage = FakeBatchedStage()
    res = pipeline.embed_images(imgs, [_wm(i) for i in range(len(imgs))], True, {"block_size": 8}, workers=3, device_stage=stage,
                                batch_images=k)
    assert stage.groups == groups
    assert len(res) == len(imgs)
    for i, (src, r) in enumerate(zip(imgs, res)):
        ref = pipeline._decode(src).copy()
        g = next(n for n, grp in enumerate(groups) if i in grp)
        assert tuple(r.pixels[0, 0]) == (i, g, groups[g].index(i))  # watermark index i went with image i
        ref[0, 0] = r.pixels[0, 0]
        assert np.array_equal(r.pixels, ref), i  # input order
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(r.png))), ref), i
    # one watermark for all: the same grouping
    stage = FakeBatchedStage()
    pipeline.embed_images(imgs, _wm(0), True, None, device_stage=stage, batch_images=k)
    assert stage.groups == groups


def test_pipeline_batch_images_errors_and_none():
    imgs = _images(SIZES[:4])
    with pytest.raises(ValueError, match="3 watermarks for 4 images"):
        pipeline.embed_images(imgs, [_wm(i) for i in range(3)], device_stage=FakeBatchedStage(), batch_images=2)
    with pytest.raises(ValueError, match="batch_images"):
        pipeline.embed_images(imgs, _wm(0), device_stage=FakeBatchedStage(), batch_images=0)

    class Short(FakeBatchedStage):
        def __call__(self, rgbs, indices):
            return super().__call__(rgbs, indices)[:-1]

    with pytest.raises(ValueError, match="results"):
        pipeline.embed_images(imgs, _wm(0), device_stage=Short(), batch_images=2)

    # batch_images=None: today's per-image calls, the batched form is never used
    calls = []

    def per_image(rgb, *index):
        assert isinstance(rgb, np.ndarray) and rgb.ndim == 3
        calls.append(index)
        return rgb, None

    pipeline.embed_images(imgs, _wm(0), device_stage=per_image)
    assert calls == [()] * 4
    calls.clear()
    pipeline.embed_images(imgs, [_wm(i) for i in range(4)], device_stage=per_image, batch_images=None)
    assert calls == [(0,), (1,), (2,), (3,)]
    assert issubclass(pipeline.RaggedGpuStage, pipeline.GpuStage)
