"""Ragged keyed extraction on the CPU: tmfwm_sigma1_map_ragged / tmfwm_extract_keyed_ragged are
exported and declared, their arguments are checked before any device call, a valid call without
a GPU fails with TMFWM_ERR_NODEVICE, the Python layer refuses what it must before it looks at a
device, and pipeline.extract_images groups images for a batched device stage.  No compute runs
here."""
import ctypes
import io

import numpy as np
import pytest
from PIL import Image

from thatsmyface_amd import _lib, pipeline


def test_symbols_exported_and_declared():
    L = _lib.load()
    assert hasattr(L, "tmfwm_sigma1_map_ragged") and hasattr(L, "tmfwm_extract_keyed_ragged")
    res, args = _lib.SIGNATURES["tmfwm_sigma1_map_ragged"]
    assert res is ctypes.c_int and len(args) == 7  # no alpha
    res, args = _lib.SIGNATURES["tmfwm_extract_keyed_ragged"]
    assert res is ctypes.c_int and len(args) == 8 and args[3] is ctypes.c_double
    assert L.tmfwm_abi_version() == _lib.ABI_VERSION == 10
    # the descriptors' layout as in include/tmfwm.h
    assert ctypes.sizeof(_lib.KeyFrame) == 24 and ctypes.sizeof(_lib.KeyedFrame) == 32
    assert [f[0] for f in _lib.KeyFrame._fields_] == ["rgb", "out_key", "height", "width"]
    assert [f[0] for f in _lib.KeyedFrame._fields_] == ["wm_rgb", "key", "out_tile", "height", "width"]
    assert _lib.KeyFrame.height.offset == 16 and _lib.KeyedFrame.height.offset == 24


def _calls():
    """(map, keyed, their descriptor arrays): callables over two valid 16 x 16 descriptors; the
    float buffers are 16-byte aligned views so that + 1 and + 2 are the misaligned addresses."""
    L = _lib.load()
    a = np.zeros((16, 16, 3), np.uint8)
    t = np.zeros((2, 2), np.uint8)
    raw = np.zeros(64 + 16, np.uint8)
    off = (-raw.ctypes.data) % 16
    key = raw[off:off + 16].view(np.float32).reshape(2, 2)
    kout = raw[off + 32:off + 48].view(np.float32).reshape(2, 2)
    assert key.ctypes.data % 16 == 0 and kout.ctypes.data % 16 == 0
    keep = (a, t, raw, key, kout)
    md = (_lib.KeyFrame * 2)(_lib.KeyFrame(a.ctypes.data, kout.ctypes.data, 16, 16), _lib.KeyFrame(a.ctypes.data, kout.ctypes.data, 16, 16))
    kd = (_lib.KeyedFrame * 2)(_lib.KeyedFrame(a.ctypes.data, key.ctypes.data, t.ctypes.data, 16, 16),
                               _lib.KeyedFrame(a.ctypes.data, key.ctypes.data, t.ctypes.data, 16, 16))

    def smap(block=8, alpha=None, mem=_lib.MEM_HOST, route=0, n=2, desc=md, _k=keep):
        return L.tmfwm_sigma1_map_ragged(ctypes.addressof(desc) if desc is not None else None, n, block, mem, None, route, None)

    def keyed(block=8, alpha=0.1, mem=_lib.MEM_HOST, route=0, n=2, desc=kd, _k=keep):
        return L.tmfwm_extract_keyed_ragged(ctypes.addressof(desc) if desc is not None else None, n, block, alpha, mem, None, route, None)

    return smap, keyed, md, kd


MEMS = (_lib.MEM_HOST, _lib.MEM_DEVICE)


def test_argument_validation_before_device():
    smap, keyed, md, kd = _calls()
    for call in (smap, keyed):
        for mem in MEMS:
            assert call(n=2, desc=None, mem=mem) == _lib.ERR_INVALID and "NULL" in _lib.last_error()  # NULL array with n > 0
            assert call(n=-1, mem=mem) == _lib.ERR_INVALID  # negative count
            for bad_block in (7, 18, 2):
                assert call(block=bad_block, mem=mem) == _lib.ERR_UNSUPPORTED
            for bad_route in (-1, 4):
                assert call(route=bad_route, mem=mem) == _lib.ERR_INVALID and "route" in _lib.last_error()
            for rank1 in (_lib.ROUTE_RANK1, _lib.ROUTE_RANK1_REFERENCE):
                assert call(route=rank1, mem=mem) == _lib.ERR_UNSUPPORTED and "rank-1" in _lib.last_error()
        for bad_mem in (-1, 2):
            assert call(mem=bad_mem) == _lib.ERR_INVALID and "mem_kind" in _lib.last_error()
    for mem in MEMS:
        for alpha in (float("nan"), float("inf"), 0.0):
            assert keyed(alpha=alpha, mem=mem) == _lib.ERR_INVALID and "alpha" in _lib.last_error()
    # inside a descriptor, in the second frame, for both memory kinds
    for mem in MEMS:
        for field in ("height", "width"):
            for desc, call in ((md, smap), (kd, keyed)):
                old = getattr(desc[1], field)
                setattr(desc[1], field, -3)
                assert call(mem=mem) == _lib.ERR_INVALID and "frame 1" in _lib.last_error(), (mem, field)
                setattr(desc[1], field, old)
        for desc, call, fields in ((md, smap, ("rgb", "out_key")), (kd, keyed, ("wm_rgb", "key", "out_tile"))):
            for field in fields:
                old = getattr(desc[1], field)
                setattr(desc[1], field, None)
                assert call(mem=mem) == _lib.ERR_INVALID and "NULL" in _lib.last_error(), (mem, field)
                setattr(desc[1], field, old)
        # a key at an odd address, and one at + 2
        for desc, call, field in ((md, smap, "out_key"), (kd, keyed, "key")):
            old = getattr(desc[1], field)
            for shift in (1, 2):
                setattr(desc[1], field, old + shift)
                assert call(mem=mem) == _lib.ERR_INVALID, (mem, field, shift)
                assert "frame 1" in _lib.last_error() and "aligned" in _lib.last_error() and field in _lib.last_error()
            setattr(desc[1], field, old)
    # a frame without a block needs no key and no output pointer; one of zero height no pointer at all
    md[1].out_key, md[1].height = None, 7
    kd[1].key, kd[1].out_tile, kd[1].width = None, None, 5
    for call in (smap, keyed):
        for mem in MEMS:
            assert call(mem=mem) in (0, _lib.ERR_NODEVICE), _lib.last_error()
    md[1].out_key, md[1].height = 1, 7  # nor is a misaligned one looked at
    assert smap() in (0, _lib.ERR_NODEVICE), _lib.last_error()
    md[1].rgb, md[1].out_key, md[1].height = None, None, 0
    kd[1].wm_rgb, kd[1].height = None, 0
    for call in (smap, keyed):
        assert call() in (0, _lib.ERR_NODEVICE), _lib.last_error()


def test_valid_call_needs_a_device():
    """Without a GPU a valid call fails with TMFWM_ERR_NODEVICE (no CPU fallback); with one it runs."""
    smap, keyed, _, _ = _calls()
    if _lib.device_count() > 0:
        assert smap() == 0 and keyed() == 0, _lib.last_error()
        return
    for call in (smap, keyed):
        for mem in MEMS:
            assert call(mem=mem) == _lib.ERR_NODEVICE and "no HIP device" in _lib.last_error()
        assert call(n=0, desc=None) == _lib.ERR_NODEVICE


def test_python_layer_refuses_before_any_device_work():
    batch = pytest.importorskip("thatsmyface_amd.batch")
    torch = pytest.importorskip("torch")
    for route in ("rank1", "rank1_reference"):
        with pytest.raises(NotImplementedError, match="rank-1"):
            batch.sigma1_map_ragged([object()], 8, route=route)  # no tensor is looked at
        with pytest.raises(NotImplementedError, match="rank-1"):
            batch.extract_keyed_ragged([object()], [object()], 8, 0.1, route=route)
    with pytest.raises(NotImplementedError):
        batch.sigma1_map_ragged([], 7)
    with pytest.raises(NotImplementedError):
        batch.extract_keyed_ragged([], [], 18, 0.1)
    frame = torch.zeros((24, 40, 3), dtype=torch.uint8)
    with pytest.raises(TypeError, match="float32"):
        batch.extract_keyed_ragged([frame], [torch.zeros((3, 5), dtype=torch.float64)], 8, 0.1)
    with pytest.raises(TypeError, match="float32"):
        batch.extract_keyed_ragged([frame], [np.zeros((3, 5), np.float32)], 8, 0.1)
    for shape in ((5, 3), (3, 4), (1, 3, 5), (15,)):
        with pytest.raises(ValueError, match="one block size and one image size"):
            batch.extract_keyed_ragged([frame], [torch.zeros(shape, dtype=torch.float32)], 8, 0.1)
    with pytest.raises(ValueError, match="one block size and one image size"):  # the key of another block size
        batch.extract_keyed_ragged([frame], [torch.zeros((6, 10), dtype=torch.float32)], 8, 0.1)
    with pytest.raises(ValueError, match="keys for"):
        batch.extract_keyed_ragged([frame, frame], [torch.zeros((3, 5), dtype=torch.float32)], 8, 0.1)
    assert batch.sigma1_map_ragged([], 8) == [] and batch.extract_keyed_ragged([], [], 8, 0.1) == []
    st = {}
    assert batch.extract_keyed_ragged([], [], 8, 0.1, stats=st) == [] and st == {"lapack_blocks": 0, "list_pass_blocks": 0}


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


class FakeKeyedStage:
    """Each image's "tile" records where it went: (index, group number, place in the group,
    its key's [0, 0] entry) in the first four bytes of an (H // 8, W // 8) tile."""

    def __init__(self):
        self.groups = []

    def __call__(self, rgbs, keys, indices):
        assert len(rgbs) == len(keys) == len(indices)
        g = len(self.groups)
        self.groups.append(list(indices))
        out, waited = [], []
        for k, (rgb, key, i) in enumerate(zip(rgbs, keys, indices)):
            t = np.zeros((rgb.shape[0] // 8, rgb.shape[1] // 8), np.uint8)
            t.reshape(-1)[:4] = (i, g, k, int(key[0, 0]))
            out.append((t, (lambda w=waited, i=i: w.append(i)) if i % 2 else None))
        return out


SIZES = [(16, 24), (9, 40), (16, 24), (33, 17), (8, 32), (24, 24), (16, 31)]


def _keys(sizes, b=8):
    return [np.full((h // b, w // b), 100 + i, np.float32) for i, (h, w) in enumerate(sizes)]


@pytest.mark.parametrize("k,groups", [(3, [[0, 1, 2], [3, 4, 5], [6]]), (1, [[i] for i in range(7)]), (7, [list(range(7))]),
                                      (50, [list(range(7))])])
def test_pipeline_groups_in_order(k, groups):
    imgs, keys = _images(SIZES), _keys(SIZES)
    stage = FakeKeyedStage()
    res = list(pipeline.extract_images(imgs, keys, {"block_size": 8}, batch_images=k, workers=3, device_stage=stage))
    assert stage.groups == groups
    assert len(res) == len(imgs)
    for i, ((h, w), r) in enumerate(zip(SIZES, res)):
        assert isinstance(r, Image.Image) and r.mode == "L" and r.size == (w // 8, h // 8), i
        g = next(n for n, grp in enumerate(groups) if i in grp)
        assert list(np.asarray(r).reshape(-1)[:4]) == [i, g, groups[g].index(i), 100 + i], i  # key i went with image i, input order


def test_pipeline_errors_raise_before_the_group_reaches_the_stage():
    imgs, keys = _images(SIZES[:4]), _keys(SIZES[:4])
    with pytest.raises(ValueError, match="3 keys for 4 images"):
        pipeline.extract_images(imgs, keys[:3], device_stage=FakeKeyedStage())
    for bad in (0, None):
        with pytest.raises(ValueError, match="batch_images"):
            pipeline.extract_images(imgs, keys, device_stage=FakeKeyedStage(), batch_images=bad)
    # the second group holds the bad key: the first group runs, the second never reaches the stage
    for wrong, err in ((np.zeros((4, 2), np.float64), TypeError), (np.zeros((2, 4), np.float32), ValueError),
                       (np.zeros((33 // 4, 17 // 4), np.float32), ValueError)):
        stage = FakeKeyedStage()
        it = pipeline.extract_images(imgs, keys[:3] + [wrong], {"block_size": 8}, batch_images=2, device_stage=stage)
        with pytest.raises(err, match="float32" if err is TypeError else "one block size and one image size"):
            list(it)
        assert stage.groups == [[0, 1]]

    class Short(FakeKeyedStage):
        def __call__(self, rgbs, keys, indices):
            return super().__call__(rgbs, keys, indices)[:-1]

    with pytest.raises(ValueError, match="results"):
        list(pipeline.extract_images(imgs, keys, device_stage=Short(), batch_images=2))
    assert list(pipeline.extract_images([], [], device_stage=FakeKeyedStage())) == []
