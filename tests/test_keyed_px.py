"""The keyed calls with a pixel layout on the CPU: tmfwm_sigma1_map_px, tmfwm_extract_keyed_px,
tmfwm_embed_key_px, tmfwm_sigma1_map_ragged_px and tmfwm_extract_keyed_ragged_px are exported and
declared, their arguments are checked before any device call, a valid call without a GPU fails
with TMFWM_ERR_NODEVICE, and the Python layer refuses a ragged list that mixes 3- and 4-byte
frames before it looks at a device.  No compute runs here."""
import ctypes
import os
import re

import numpy as np
import pytest

from thatsmyface_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tmfwm_sigma1_map_px", "tmfwm_extract_keyed_px", "tmfwm_embed_key_px", "tmfwm_sigma1_map_ragged_px",
       "tmfwm_extract_keyed_ragged_px")
MEMS = (_lib.MEM_HOST, _lib.MEM_DEVICE)
H, W, B = 16, 24, 8
NBH, NBW = H // B, W // B
KB = NBH * NBW * 4  # bytes of one key


def test_symbols_exported_and_declared():
    L = _lib.load()
    with open(os.path.join(ROOT, "include", "tmfwm.h")) as f:
        header = f.read()
    for name in NEW:
        assert hasattr(L, name), name
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int
        m = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert m, f"{name} is not declared in include/tmfwm.h"
        assert len(args) == m.group(1).count(",") + 1, name  # one ctypes type per declared parameter
    # the sibling's arguments, plus the pixel size (and the stride moved beside it)
    assert len(_lib.SIGNATURES["tmfwm_sigma1_map_px"][1]) == len(_lib.SIGNATURES["tmfwm_sigma1_map"][1]) + 1
    assert len(_lib.SIGNATURES["tmfwm_extract_keyed_px"][1]) == len(_lib.SIGNATURES["tmfwm_extract_keyed"][1]) + 1
    assert len(_lib.SIGNATURES["tmfwm_embed_key_px"][1]) == len(_lib.SIGNATURES["tmfwm_embed_tiles"][1]) + 2
    assert len(_lib.SIGNATURES["tmfwm_sigma1_map_ragged_px"][1]) == len(_lib.SIGNATURES["tmfwm_sigma1_map_ragged"][1]) + 1
    assert len(_lib.SIGNATURES["tmfwm_extract_keyed_ragged_px"][1]) == len(_lib.SIGNATURES["tmfwm_extract_keyed_ragged"][1]) + 1
    assert L.tmfwm_abi_version() == _lib.ABI_VERSION == 10  # added within ABI 10
    assert (_lib.PIX_RGB, _lib.PIX_RGBX) == (3, 4)


class Calls:
    """The five entries over valid two-frame arguments (16 x 24 frames, block 8); every keyword
    replaces one argument.  The float buffers are 16-byte aligned views, so + 1 and + 2 are the
    misaligned addresses."""

    def __init__(self):
        self.L = _lib.load()
        self.frames = np.zeros((2, H, W, 4), np.uint8)  # large enough for either layout
        self.out = np.zeros((2, H, W, 4), np.uint8)
        self.tiles = np.zeros((2, NBH, NBW), np.uint8)
        raw = np.zeros(3 * 64 + 16, np.uint8)
        off = (-raw.ctypes.data) % 16
        self.key = raw[off:off + 2 * KB].view(np.float32)
        self.kout = raw[off + 64:off + 64 + 2 * KB].view(np.float32)
        self.kout2 = raw[off + 128:off + 128 + 2 * KB].view(np.float32)
        self.raw = raw
        assert self.key.ctypes.data % 16 == 0 and self.kout.ctypes.data % 16 == 0
        p = self.frames.ctypes.data
        self.md = (_lib.KeyFrame * 2)(_lib.KeyFrame(p, self.kout.ctypes.data, H, W), _lib.KeyFrame(p, self.kout2.ctypes.data, H, W))
        self.kd = (_lib.KeyedFrame * 2)(_lib.KeyedFrame(p, self.key.ctypes.data, self.tiles.ctypes.data, H, W),
                                        _lib.KeyedFrame(p, self.key.ctypes.data, self.tiles[1].ctypes.data, H, W))

    def smap(self, px=4, stride=None, out_key=None, mem=_lib.MEM_HOST, route=0, block=B, **_):
        return self.L.tmfwm_sigma1_map_px(self.frames.ctypes.data, px, H * W * px if stride is None else stride, 2, H, W, block,
                                          self.kout.ctypes.data if out_key is None else out_key, mem, None, route, None)

    def keyed(self, px=4, stride=None, key=None, key_stride=KB, mem=_lib.MEM_HOST, route=0, block=B, alpha=0.1, **_):
        return self.L.tmfwm_extract_keyed_px(self.frames.ctypes.data, px, H * W * px if stride is None else stride, 2, H, W,
                                             self.key.ctypes.data if key is None else key, key_stride, block, alpha,
                                             self.tiles.ctypes.data, mem, None, route, None)

    def embed(self, px=4, stride=None, opx=4, ostride=None, out_key=None, key_stride=KB, mem=_lib.MEM_HOST, route=0, block=B,
              alpha=0.1, **_):
        return self.L.tmfwm_embed_key_px(self.frames.ctypes.data, px, H * W * px if stride is None else stride, 2, H, W,
                                         self.tiles.ctypes.data, NBH * NBW, block, alpha, self.out.ctypes.data, opx,
                                         H * W * opx if ostride is None else ostride,
                                         self.kout.ctypes.data if out_key is None else out_key, key_stride, mem, None, route, None)

    def rmap(self, px=4, mem=_lib.MEM_HOST, route=0, block=B, **_):
        return self.L.tmfwm_sigma1_map_ragged_px(ctypes.addressof(self.md), 2, block, px, mem, None, route, None)

    def rkeyed(self, px=4, mem=_lib.MEM_HOST, route=0, block=B, alpha=0.1, **_):
        return self.L.tmfwm_extract_keyed_ragged_px(ctypes.addressof(self.kd), 2, block, alpha, px, mem, None, route, None)

    def all(self):
        return (self.smap, self.keyed, self.embed, self.rmap, self.rkeyed)


def test_pixel_bytes_checked_before_device():
    c = Calls()
    for call in c.all():
        for mem in MEMS:
            for px in (0, 2, 5, -3):
                assert call(px=px, stride=H * W * 4, mem=mem) == _lib.ERR_INVALID, (call.__name__, px, mem)
                assert "pixel bytes" in _lib.last_error(), _lib.last_error()
    for mem in MEMS:  # the output side of the enrolment call alike
        for opx in (0, 2, 5):
            assert c.embed(opx=opx, ostride=H * W * 4, mem=mem) == _lib.ERR_INVALID and "pixel bytes" in _lib.last_error()


def test_frame_stride_checked_before_device():
    c = Calls()
    for call in (c.smap, c.keyed, c.embed):
        for mem in MEMS:
            assert call(px=4, stride=H * W * 4 - 1, mem=mem) == _lib.ERR_INVALID, (call.__name__, mem)
            assert "frame_stride" in _lib.last_error(), _lib.last_error()
            # a stride that holds 3-byte frames does not hold 4-byte ones; at 3 it is enough
            assert call(px=4, stride=H * W * 3, mem=mem) == _lib.ERR_INVALID and "frame_stride" in _lib.last_error()
            assert call(px=3, stride=H * W * 3 - 1, mem=mem) == _lib.ERR_INVALID and "frame_stride" in _lib.last_error()
    for mem in MEMS:
        assert c.embed(opx=4, ostride=H * W * 4 - 1, mem=mem) == _lib.ERR_INVALID and "frame_stride" in _lib.last_error()


def test_key_stride_and_alignment_checked_before_device():
    c = Calls()
    for mem in MEMS:
        for px in (3, 4):
            for bad in (KB - 4, KB + 2, -4):
                assert c.keyed(px=px, key_stride=bad, mem=mem) == _lib.ERR_INVALID and "key_stride" in _lib.last_error(), (px, bad)
            for bad in (KB - 4, KB + 2, 0, -4):  # the enrolment call writes a key per frame: no shared key
                for opx in (3, 4):
                    assert c.embed(px=px, opx=opx, key_stride=bad, mem=mem) == _lib.ERR_INVALID, (px, opx, bad)
                    assert "key_stride" in _lib.last_error(), _lib.last_error()
            for shift in (1, 2):
                assert c.smap(px=px, out_key=c.kout.ctypes.data + shift, mem=mem) == _lib.ERR_INVALID, (px, shift, mem)
                assert "out_key" in _lib.last_error() and "aligned" in _lib.last_error()
                assert c.keyed(px=px, key=c.key.ctypes.data + shift, mem=mem) == _lib.ERR_INVALID, (px, shift, mem)
                assert "key" in _lib.last_error() and "aligned" in _lib.last_error()
                for opx in (3, 4):
                    assert c.embed(px=px, opx=opx, out_key=c.kout.ctypes.data + shift, mem=mem) == _lib.ERR_INVALID, (px, opx, shift)
                    assert "out_key" in _lib.last_error() and "aligned" in _lib.last_error()
        # ragged: inside the second descriptor, naming the frame
        for px in (3, 4):
            for desc, call, field in ((c.md, c.rmap, "out_key"), (c.kd, c.rkeyed, "key")):
                old = getattr(desc[1], field)
                for shift in (1, 2):
                    setattr(desc[1], field, old + shift)
                    assert call(px=px, mem=mem) == _lib.ERR_INVALID, (px, field, shift, mem)
                    assert "frame 1" in _lib.last_error() and "aligned" in _lib.last_error() and field in _lib.last_error()
                setattr(desc[1], field, old)


def test_other_arguments_as_the_siblings():
    c = Calls()
    for call in c.all():
        for mem in MEMS:
            for bad_block in (7, 18, 2):
                assert call(block=bad_block, mem=mem) == _lib.ERR_UNSUPPORTED, call.__name__
            for bad_route in (-1, 4):
                assert call(route=bad_route, mem=mem) == _lib.ERR_INVALID and "route" in _lib.last_error()
    for call in (c.embed, c.rmap, c.rkeyed):  # (the single-size map and extract look at mem_kind after the device, as their siblings)
        for bad_mem in (-1, 2):
            assert call(mem=bad_mem) == _lib.ERR_INVALID and "mem_kind" in _lib.last_error(), call.__name__
    for call in (c.rmap, c.rkeyed):  # the rank-1 routes stay refused on ragged calls, at either pixel size
        for px in (3, 4):
            for rank1 in (_lib.ROUTE_RANK1, _lib.ROUTE_RANK1_REFERENCE):
                assert call(px=px, route=rank1) == _lib.ERR_UNSUPPORTED and "rank-1" in _lib.last_error()
    for call in (c.keyed, c.rkeyed):
        for alpha in (float("nan"), float("inf"), 0.0):
            assert call(alpha=alpha) == _lib.ERR_INVALID and "alpha" in _lib.last_error()
    assert c.embed(alpha=float("nan")) == _lib.ERR_INVALID and "alpha" in _lib.last_error()


def test_valid_call_needs_a_device():
    """Without a GPU a valid call fails with TMFWM_ERR_NODEVICE (no CPU fallback); with one it runs."""
    c = Calls()
    gpu = _lib.device_count() > 0
    for call in c.all():
        for px in (3, 4):
            if gpu:
                assert call(px=px) == 0, (call.__name__, px, _lib.last_error())
                continue
            for mem in MEMS:
                assert call(px=px, mem=mem) == _lib.ERR_NODEVICE, (call.__name__, px, mem, _lib.last_error())
                assert "no HIP device" in _lib.last_error()
    if not gpu:
        for px, opx in ((3, 4), (4, 3), (3, 3)):
            assert c.embed(px=px, opx=opx) == _lib.ERR_NODEVICE, (px, opx, _lib.last_error())
        assert c.smap(px=4, stride=H * W * 4 + 3) == _lib.ERR_NODEVICE  # a padded stride, not a multiple of 4, is valid


def test_python_layer_refuses_a_layout_mix_before_any_device_work():
    batch = pytest.importorskip("thatsmyface_amd.batch")
    torch = pytest.importorskip("torch")
    f3 = torch.zeros((24, 40, 3), dtype=torch.uint8)
    f4 = torch.zeros((24, 40, 4), dtype=torch.uint8)
    k = torch.zeros((3, 5), dtype=torch.float32)
    for frames in ([f3, f4], [f4, f3], [f4, f4, f3]):
        with pytest.raises(ValueError, match="mixes 3- and 4-byte pixels"):
            batch.sigma1_map_ragged(frames, 8)
        with pytest.raises(ValueError, match="mixes 3- and 4-byte pixels"):
            batch.extract_keyed_ragged(frames, [k] * len(frames), 8, 0.1)
    # the calls that write pixels keep refusing 4-byte frames (the mix is not what they complain about)
    with pytest.raises(ValueError, match="GPU tensor|\\(H, W, 3\\)"):
        batch.embed_ragged([f4], [torch.zeros((3, 5), dtype=torch.uint8)], 8)
    with pytest.raises(ValueError, match="GPU tensor|\\(H, W, 3\\)"):
        batch.extract_ragged([f4], [f4], 8)
    for px in (2, 5):  # neither layout
        bad = torch.zeros((24, 40, px), dtype=torch.uint8)
        with pytest.raises(ValueError):
            batch.sigma1_map_ragged([bad], 8)
