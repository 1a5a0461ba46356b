"""The ragged calls with one alpha per frame, on the CPU: the four tmfwm_*_ragged_alphas entries
are exported, declared and typed; every argument check answers before the device; a call without
a frame is TMFWM_OK and a valid one needs a device; batch.* refuses an alpha sequence of the wrong
length before it looks at a tensor; and the pipeline, with a fake stage, splits a group by
(block_size, svd_route), keeps input order, hands each part its alphas and is unchanged for a
single dict.  No compute runs here."""
import ctypes
import io
import os
import re

import numpy as np
import pytest
from PIL import Image

from thatsmyface_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tmfwm_embed_ragged_alphas", "tmfwm_embed_key_ragged_alphas", "tmfwm_extract_ragged_alphas",
         "tmfwm_extract_keyed_ragged_alphas")
NAN, INF = float("nan"), float("inf")


def test_symbols_exported_declared_and_typed():
    L = _lib.load()
    with open(os.path.join(ROOT, "include", "tmfwm.h")) as f:
        header = f.read()
    for name in NAMES:
        assert hasattr(L, name), name
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, f"{name} is not declared in include/tmfwm.h"
        params = [p.strip() for p in m.group(1).split(",")]
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(params), name
        # the declared parameter types against the ctypes ones
        for p, a in zip(params, args):
            want = (ctypes.c_void_p if "*" in p else ctypes.c_int64 if p.startswith("int64_t") else ctypes.c_int32
                    if p.startswith("int32_t") else None)
            assert a is want, (name, p)
        assert params[1].startswith("const double *alphas") and params[2] == "int64_t n_frames", name
    assert len(_lib.SIGNATURES["tmfwm_extract_keyed_ragged_alphas"][1]) == 9  # pixel_bytes
    assert L.tmfwm_abi_version() == _lib.ABI_VERSION == 10  # new entry points within ABI 10


def _calls():
    """The four entries over two valid 16 x 16 descriptors in host memory."""
    L = _lib.load()
    a = np.zeros((16, 16, 3), np.uint8)
    a4 = np.zeros((16, 16, 4), np.uint8)
    o = np.empty_like(a)
    t = np.zeros((2, 2), np.uint8)
    to = np.zeros((2, 2), np.uint8)
    k = np.ones((2, 2), np.float32)
    ko = np.zeros((2, 2), np.float32)
    keep = (a, a4, o, t, to, k, ko)
    descs = {
        "embed": (_lib.EmbedFrame * 2)(*[_lib.EmbedFrame(a.ctypes.data, o.ctypes.data, t.ctypes.data, 16, 16) for _ in range(2)]),
        "embed_key": (_lib.EmbedKeyFrame * 2)(*[_lib.EmbedKeyFrame(a.ctypes.data, o.ctypes.data, t.ctypes.data, ko.ctypes.data, 16, 16)
                                                for _ in range(2)]),
        "extract": (_lib.ExtractFrame * 2)(*[_lib.ExtractFrame(a.ctypes.data, a.ctypes.data, to.ctypes.data, 16, 16) for _ in range(2)]),
        "keyed": (_lib.KeyedFrame * 2)(*[_lib.KeyedFrame(a4.ctypes.data, k.ctypes.data, to.ctypes.data, 16, 16) for _ in range(2)]),
    }
    fns = {"embed": L.tmfwm_embed_ragged_alphas, "embed_key": L.tmfwm_embed_key_ragged_alphas,
           "extract": L.tmfwm_extract_ragged_alphas, "keyed": L.tmfwm_extract_keyed_ragged_alphas}

    def make(kind):
        def call(alphas=(0.1, 0.2), block=8, mem=_lib.MEM_HOST, route=_lib.ROUTE_HYBRID, n=2, desc=descs[kind], px=4, _k=keep):
            arr = None if alphas is None else (ctypes.c_double * max(len(alphas), 1))(*alphas)
            head = (ctypes.addressof(desc) if desc is not None else None, ctypes.addressof(arr) if arr is not None else None, n, block)
            tail = (mem, None, route, None)
            return fns[kind](*head, *((px,) if kind == "keyed" else ()), *tail)

        return call

    return {kind: make(kind) for kind in fns}, descs


def test_argument_validation_before_device():
    calls, _ = _calls()
    for kind, call in calls.items():
        extract = kind in ("extract", "keyed")
        assert call(alphas=None) == _lib.ERR_INVALID and "alphas is NULL" in _lib.last_error(), kind
        assert call(desc=None) == _lib.ERR_INVALID and "NULL" in _lib.last_error(), kind
        assert call(n=-1) == _lib.ERR_INVALID, kind
        # every alpha, the first and the last
        for bad in (NAN, INF, -INF) + ((0.0, -0.0) if extract else ()):
            for at in (0, 1):
                alphas = [0.1, 0.2]
                alphas[at] = bad
                for mem in (_lib.MEM_HOST, _lib.MEM_DEVICE):
                    assert call(alphas=alphas, mem=mem) == _lib.ERR_INVALID, (kind, bad, at)
                    assert f"frame {at}" in _lib.last_error() and "alpha" in _lib.last_error(), (kind, bad, at, _lib.last_error())
        if not extract:  # zero is an alpha of the embeds
            assert call(alphas=[0.0, 0.1]) in (0, _lib.ERR_NODEVICE), _lib.last_error()
        for bad_route in (-1, 4):
            assert call(route=bad_route) == _lib.ERR_INVALID and "route" in _lib.last_error(), kind
        for route in (_lib.ROUTE_RANK1, _lib.ROUTE_RANK1_REFERENCE):
            if extract:  # the extracts take the hybrid and the reference route
                assert call(route=route) == _lib.ERR_UNSUPPORTED, kind
            else:
                assert call(route=route) in (0, _lib.ERR_NODEVICE), _lib.last_error()
        for bad_block in (7, 18, 2):
            assert call(block=bad_block) == _lib.ERR_UNSUPPORTED, kind
        for bad_mem in (-1, 2):
            assert call(mem=bad_mem) == _lib.ERR_INVALID and "mem_kind" in _lib.last_error(), kind
    for bad_px in (0, 2, 5):
        assert calls["keyed"](px=bad_px) == _lib.ERR_INVALID and "pixel bytes" in _lib.last_error()
    assert calls["keyed"](px=3) in (0, _lib.ERR_NODEVICE), _lib.last_error()


def test_alpha_of_a_frame_without_a_block_is_checked():
    """Every entry is checked, whether or not its frame has a block (here: 7 rows, and no pixel at all)."""
    calls, descs = _calls()
    for kind, call in calls.items():
        for height in (7, 0):
            descs[kind][1].height = height
            assert call(alphas=[0.1, NAN]) == _lib.ERR_INVALID and "frame 1" in _lib.last_error(), (kind, height)
        descs[kind][1].height = 16


def test_descriptor_checks_name_the_frame():
    calls, descs = _calls()
    for kind, call in calls.items():
        descs[kind][1].width = -3
        assert call() == _lib.ERR_INVALID and "frame 1" in _lib.last_error(), kind
        descs[kind][1].width = 16


def test_no_frame_is_ok_and_a_valid_call_needs_a_device():
    calls, _ = _calls()
    for kind, call in calls.items():
        assert call(n=0) == 0, (kind, _lib.last_error())
        assert call(n=0, desc=None, alphas=None) == 0, (kind, _lib.last_error())
        assert call(n=0, block=7) == _lib.ERR_UNSUPPORTED, kind  # the other arguments are still checked
    if _lib.device_count() > 0:
        for kind, call in calls.items():
            assert call() == 0, (kind, _lib.last_error())
        return
    for kind, call in calls.items():
        for mem in (_lib.MEM_HOST, _lib.MEM_DEVICE):
            assert call(mem=mem) == _lib.ERR_NODEVICE and "no HIP device" in _lib.last_error(), kind


def test_batch_refuses_wrong_alpha_count_before_any_device_work():
    torch = pytest.importorskip("torch")
    from thatsmyface_amd import batch

    f = [torch.zeros((16, 16, 3), dtype=torch.uint8) for _ in range(3)]  # CPU tensors: a device check would refuse them
    t = [torch.zeros((2, 2), dtype=torch.uint8) for _ in range(3)]
    k = [torch.zeros((2, 2), dtype=torch.float32) for _ in range(3)]
    for bad in ([0.1, 0.2], [0.1] * 4, [], (0.1,), np.array([0.1, 0.2])):
        for fn, args in ((batch.embed_ragged, (f, t)), (batch.embed_ragged_rank1, (f, t)), (batch.embed_with_key_ragged, (f, t)),
                         (batch.embed_with_key_ragged_rank1, (f, t)), (batch.extract_ragged, (f, f)),
                         (batch.extract_keyed_ragged, (f, k))):
            with pytest.raises(ValueError, match=f"{len(bad)} alphas for 3 frames"):
                fn(*args, 8, bad)
    with pytest.raises(ValueError, match="2 alphas for 3 frames"):
        batch.embed_ragged(f, t, 8, (a for a in (0.1, 0.2)))  # any iterable is a sequence of alphas
    with pytest.raises(TypeError, match="alpha must be a number or a sequence"):
        batch.embed_ragged(f, t, 8, None)
    # the right count gets as far as the tensors (not on a GPU); a number in any dress likewise
    for alpha in ([0.1, 0.2, 0.3], torch.tensor([0.1, 0.2, 0.3]), 0.1, 1, np.float32(0.1), np.array(0.1), torch.tensor(0.1)):
        with pytest.raises(ValueError, match="must be a GPU tensor"):
            batch.embed_ragged(f, t, 8, alpha)
        with pytest.raises(ValueError, match="must be a GPU tensor"):
            batch.extract_keyed_ragged(f, k, 8, alpha)


# ---- the pipeline with a fake stage

def _png(arr):
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, format="PNG")
    return buf.getvalue()


def _sources(n):
    rng = np.random.default_rng(3)
    return [rng.integers(0, 256, (16 + 2 * i, 24 + i, 3), dtype=np.uint8) for i in range(n)]


# image i's settings: three (block_size, svd_route) classes, every alpha its own
SETTINGS = [{"block_size": 8, "alpha": 0.10}, {"block_size": 4, "alpha": 0.20}, {"block_size": 8, "alpha": 0.30, "svd_route": "hybrid"},
            {"block_size": 4, "alpha": 0.40}, {"block_size": 8, "alpha": 0.50}, {"block_size": 4, "alpha": 0.60},
            {"alpha": 0.70}, {"block_size": 8, "svd_route": "hybrid", "alpha": 0.80}, None, {"block_size": 4, "alpha": 1.0}]


def _fake_pixels(rgb, index, s):
    """What the fake embed stage makes of an image: a function of the image, its index and its settings."""
    out = rgb.copy()
    out[0, 0] = (index, s["block_size"], int(round(s["alpha"] * 100)))
    out[0, 1, 0] = {"reference": 1, "hybrid": 2}.get(s["svd_route"], 9)
    return out


def test_pipeline_embed_groups_by_block_and_route(monkeypatch):
    from thatsmyface_amd import pipeline
    from thatsmyface_amd.constants import ALPHA, BLOCK_SIZE, SVD_ROUTE

    monkeypatch.delenv("TMFWM_SVD_ROUTE", raising=False)
    arrs = _sources(10)
    imgs = [_png(a) if i % 2 else Image.fromarray(a) for i, a in enumerate(arrs)]
    calls = []

    def stage(rgbs, indices, settings=None):
        calls.append((list(indices), settings))
        assert len(settings) == len(rgbs) == len(indices)
        return [(_fake_pixels(rgb, i, s), None) for rgb, i, s in zip(rgbs, indices, settings)]

    res = pipeline.embed_images(imgs, b"unused", True, SETTINGS, workers=3, device_stage=stage, batch_images=4)
    want = [pipeline._resolved(s) for s in SETTINGS]
    assert want[8] == {"block_size": BLOCK_SIZE, "alpha": ALPHA, "svd_route": SVD_ROUTE}
    assert len(res) == 10
    for i, r in enumerate(res):  # input order, each image with its own settings
        assert np.array_equal(r.pixels, _fake_pixels(arrs[i], i, want[i])), i
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(r.png))), r.pixels)
    # every part: one block size and one route, inside one group of 4, its images' alphas in its order
    seen = []
    for indices, settings in calls:
        assert len({(s["block_size"], s["svd_route"]) for s in settings}) == 1
        assert len({i // 4 for i in indices}) == 1 and indices == sorted(indices)
        assert [s["alpha"] for s in settings] == [want[i]["alpha"] for i in indices]
        assert all(s == want[i] for s, i in zip(settings, indices))
        seen += indices
    assert sorted(seen) == list(range(10))
    # as few parts as the classes allow: per group the distinct (block_size, svd_route) pairs
    parts = sum(len({(want[i]["block_size"], want[i]["svd_route"]) for i in range(g, min(g + 4, 10))}) for g in range(0, 10, 4))
    assert len(calls) == parts


def test_pipeline_embed_per_image_stage_takes_each_images_settings():
    from thatsmyface_amd import pipeline

    arrs = _sources(5)
    want = [pipeline._resolved(s) for s in SETTINGS[:5]]
    got = []

    def stage(rgb, settings=None):
        got.append(settings)
        return _fake_pixels(rgb, len(got) - 1, settings), None

    res = pipeline.embed_images([Image.fromarray(a) for a in arrs], b"unused", True, SETTINGS[:5], device_stage=stage)
    assert got == want
    for i, r in enumerate(res):
        assert np.array_equal(r.pixels, _fake_pixels(arrs[i], i, want[i]))

    # one watermark per image: the stage gets the index as before, and the settings
    got2 = []

    def stage2(rgb, i, settings=None):
        got2.append((i, settings))
        return _fake_pixels(rgb, i, settings), None

    pipeline.embed_images([Image.fromarray(a) for a in arrs], [b"w"] * 5, True, tuple(SETTINGS[:5]), device_stage=stage2)
    assert got2 == list(enumerate(want))


def test_pipeline_single_dict_is_unchanged():
    """A single dict (or None): the stage is called exactly as before, without the keyword."""
    from thatsmyface_amd import pipeline

    arrs = _sources(5)
    imgs = [Image.fromarray(a) for a in arrs]
    for settings in ({"block_size": 4, "alpha": 0.3}, None):
        groups = []

        def group_stage(rgbs, indices):  # no `settings` parameter: passing one would be a TypeError
            groups.append(list(indices))
            return [(rgb.copy(), None) for rgb in rgbs]

        res = pipeline.embed_images(imgs, b"unused", True, settings, device_stage=group_stage, batch_images=2)
        assert groups == [[0, 1], [2, 3], [4]]
        assert all(np.array_equal(r.pixels, a) for r, a in zip(res, arrs))
        res = pipeline.embed_images(imgs, b"unused", True, settings, device_stage=lambda rgb: (rgb.copy(), None))
        assert all(np.array_equal(r.pixels, a) for r, a in zip(res, arrs))
        res = pipeline.embed_images(imgs, [b"w"] * 5, True, settings, device_stage=lambda rgb, i: (rgb.copy(), None))
        assert len(res) == 5
        block = 4 if settings else 8
        keys = [np.zeros((a.shape[0] // block, a.shape[1] // block), np.float32) for a in arrs]
        kgroups = []

        def keyed_stage(rgbs, ks, indices):
            kgroups.append(list(indices))
            return [(np.full(k.shape, i, np.uint8), None) for k, i in zip(ks, indices)]

        tiles = list(pipeline.extract_images(imgs, keys, settings, batch_images=3, device_stage=keyed_stage))
        assert kgroups == [[0, 1, 2], [3, 4]]
        assert [int(np.asarray(t)[0, 0]) for t in tiles] == list(range(5))


def test_pipeline_extract_groups_by_block_and_route(monkeypatch):
    from thatsmyface_amd import pipeline

    monkeypatch.delenv("TMFWM_SVD_ROUTE", raising=False)
    arrs = _sources(10)
    want = [pipeline._resolved(s) for s in SETTINGS]
    keys = [np.full((a.shape[0] // s["block_size"], a.shape[1] // s["block_size"]), float(i), np.float32)
            for i, (a, s) in enumerate(zip(arrs, want))]
    calls = []

    def stage(rgbs, ks, indices, settings=None):
        calls.append((list(indices), settings))
        for rgb, k, i, s in zip(rgbs, ks, indices, settings):
            assert k is keys[i] and np.array_equal(rgb, arrs[i]) and s == want[i]
        return [(np.full(k.shape, int(round(s["alpha"] * 100)), np.uint8), None) for k, s in zip(ks, settings)]

    tiles = list(pipeline.extract_images([Image.fromarray(a) for a in arrs], keys, SETTINGS, batch_images=5, device_stage=stage))
    assert len(tiles) == 10
    for i, t in enumerate(tiles):  # input order; the tile's size is that of the image's own block size
        t = np.asarray(t)
        assert t.shape == keys[i].shape and (t == int(round(want[i]["alpha"] * 100))).all(), i
    for indices, settings in calls:
        assert len({(s["block_size"], s["svd_route"]) for s in settings}) == 1
        assert len({i // 5 for i in indices}) == 1 and indices == sorted(indices)
    assert sorted(i for indices, _ in calls for i in indices) == list(range(10))
    # a key that fits another block size is refused with its image's own block size in the message
    bad = list(keys)
    bad[1] = np.zeros((arrs[1].shape[0] // 8, arrs[1].shape[1] // 8), np.float32)
    with pytest.raises(ValueError, match="block size 4"):
        list(pipeline.extract_images([Image.fromarray(a) for a in arrs], bad, SETTINGS, batch_images=5, device_stage=stage))


def test_pipeline_refuses_a_settings_sequence_of_the_wrong_length():
    from thatsmyface_amd import pipeline

    imgs = [Image.fromarray(a) for a in _sources(3)]

    def never(*a, **k):
        raise AssertionError("the stage must not run")

    for bad in ([{}] * 2, [{}] * 4, [], ({},)):
        for batch_images in (None, 2):
            with pytest.raises(ValueError, match=f"{len(bad)} settings for 3 images"):
                pipeline.embed_images(imgs, b"unused", True, bad, device_stage=never, batch_images=batch_images)
        with pytest.raises(ValueError, match=f"{len(bad)} settings for 3 images"):
            pipeline.extract_images(imgs, [np.zeros((2, 3), np.float32)] * 3, bad, device_stage=never)
