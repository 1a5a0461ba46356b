"""Ragged keyed extraction on the GPU: batch.sigma1_map_ragged / extract_keyed_ragged,
tmfwm_sigma1_map_ragged / tmfwm_extract_keyed_ragged through ctypes, pipeline.extract_images.

Expected values come from tests/keyed_helpers.py (the oracle's dgesdd-route f32 S[0] per block),
from the oracle's lapack-route extract, and from the unchanged single-size calls
(batch.sigma1_map / extract_keyed / extract_batch), each run on one frame alone."""
import ctypes
import io
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
from keyed_helpers import bytes_of, key_of, sparks  # noqa: E402
from test_ragged_gpu import _cover, _desc, _dev, _frames, _mixed_specs, _u8  # noqa: E402

ALL_B = (4, 6, 8, 10, 12, 14, 16)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from thatsmyface_amd import _lib

    assert _lib.device_count() > 0
    return torch.device("cuda", 0)


def _bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _single_keyed(batch, fr, wm, b, alpha):
    """The single-size calls on every frame alone: (keys, tiles, summed map count, summed extract count);
    a frame without a block gives empty tensors and takes no call."""
    keys, tiles, cm, cx = [], [], 0, 0
    for f, w in zip(fr, wm):
        sm, sx = {}, {}
        keys.append(batch.sigma1_map(f[None], b, stats=sm)[0])
        tiles.append(batch.extract_keyed(w[None], keys[-1], b, alpha, stats=sx)[0])
        cm += sm["lapack_blocks"]
        cx += sx["lapack_blocks"]
    return keys, tiles, cm, cx


@pytest.mark.parametrize("b", ALL_B)
def test_every_slider_size_mixed_shapes(dev, b):
    """One call over test_ragged_gpu's mixed frame list: 139 x 203 four times, 203 x 139 twice,
    b x b (one block), (b-1) x 50 (no block), 37 x 61 (W % 4 != 0) and 64 x 256, each embedded
    with its own tile."""
    from thatsmyface_amd import batch

    specs = _mixed_specs(b)
    covers, tiles = _frames(specs, b, 900 + b)
    fr, tt = _dev(covers, dev), _dev(tiles, dev)
    wm = batch.embed_ragged(fr, tt, b, 0.1)
    nob = next(i for i, (_, H, W, _) in enumerate(specs) if H < b)
    nblocks = sum((H // b) * (W // b) for _, H, W, _ in specs)
    skeys, stiles, cm, cx = _single_keyed(batch, fr, wm, b, 0.1)
    pair = batch.extract_ragged(wm, fr, b, 0.1)
    sm, sx = {}, {}
    keys = batch.sigma1_map_ragged(fr, b, stats=sm)
    ext = batch.extract_keyed_ragged(wm, keys, b, 0.1, stats=sx)
    print("stats", b, sm, sx, cm, cx)
    assert sm["list_pass_blocks"] == 0 and sx["list_pass_blocks"] == 0, (sm, sx)
    # no list pass in front of the dgesdd route here: the counts may exceed the single-size ones, the bytes may not differ
    assert nblocks >= sm["lapack_blocks"] >= cm and nblocks >= sx["lapack_blocks"] >= cx, (sm, sx, cm, cx)
    for i, (kind, H, W, _) in enumerate(specs):
        assert keys[i].dtype == torch.float32 and tuple(keys[i].shape) == (H // b, W // b) and keys[i].data_ptr() % 4 == 0
        assert ext[i].dtype == torch.uint8 and tuple(ext[i].shape) == (H // b, W // b)
        assert _same_bits(keys[i], skeys[i]), (b, i)
        assert torch.equal(ext[i], pair[i]), (b, i)
        assert torch.equal(ext[i], stiles[i]), (b, i)
        if H >= b and W >= b:
            assert np.array_equal(_bits(keys[i]), _bits(key_of(covers[i], b))), (b, i)
            assert np.array_equal(ext[i].cpu().numpy(), O.extract_frame(wm[i].cpu().numpy(), covers[i], b, 0.1, route="lapack")), (b, i)
    assert keys[nob].numel() == 0 and ext[nob].numel() == 0
    # caller buffers; the frame without a block gets sentinel-filled ones that stay untouched
    kbuf = [torch.full((max(k.numel(), 6),), -7.0, dtype=torch.float32, device=dev) for k in keys]
    tbuf = [torch.full((max(t.numel(), 6),), 0xA5, dtype=torch.uint8, device=dev) for t in ext]
    rows = [(f.data_ptr(), k.data_ptr(), f.shape[0], f.shape[1]) for f, k in zip(fr, kbuf)]
    from thatsmyface_amd import _lib

    L = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    cnt = ctypes.c_int64(-1)
    md = _desc(_lib.KeyFrame, rows)
    _lib.check(L.tmfwm_sigma1_map_ragged(ctypes.addressof(md), len(rows), b, _lib.MEM_DEVICE, stream, _lib.ROUTE_REFERENCE,
                                         ctypes.addressof(cnt)), "map")
    assert cnt.value == nblocks  # the reference route: every block on the dgesdd route
    kd = _desc(_lib.KeyedFrame, [(w.data_ptr(), k.data_ptr(), t.data_ptr(), w.shape[0], w.shape[1]) for w, k, t in zip(wm, kbuf, tbuf)])
    cnt = ctypes.c_int64(-1)
    _lib.check(L.tmfwm_extract_keyed_ragged(ctypes.addressof(kd), len(rows), b, 0.1, _lib.MEM_DEVICE, stream, _lib.ROUTE_REFERENCE,
                                            ctypes.addressof(cnt)), "keyed")
    assert cnt.value == nblocks and L.tmfwm_last_list_pass_blocks() == 0
    for i in range(len(specs)):
        n = keys[i].numel()
        assert _same_bits(kbuf[i][:n].view(keys[i].shape), keys[i]), (b, i)  # keys do not depend on the route
        assert torch.equal(tbuf[i][:n].view(ext[i].shape), ext[i]), (b, i)
        assert (kbuf[i][n:] == -7.0).all() and (tbuf[i][n:] == 0xA5).all(), (b, i)  # nothing past a frame's blocks
    assert (kbuf[nob] == -7.0).all() and (tbuf[nob] == 0xA5).all()
    # through batch, the reference route's stats
    sr = {}
    rk = batch.sigma1_map_ragged(fr, b, stats=sr, route="reference")
    assert sr == {"lapack_blocks": nblocks, "list_pass_blocks": 0} and all(_same_bits(a, k) for a, k in zip(rk, keys))
    sr = {}
    rx = batch.extract_keyed_ragged(wm, keys, b, 0.1, stats=sr, route="reference")
    assert sr == {"lapack_blocks": nblocks, "list_pass_blocks": 0} and all(torch.equal(a, x) for a, x in zip(rx, ext))


def test_position_independence(dev):
    from thatsmyface_amd import batch

    for b in (8, 14):
        specs = _mixed_specs(b)
        covers, tiles = _frames(specs, b, 940 + b)
        fr, tt = _dev(covers, dev), _dev(tiles, dev)
        wm = batch.embed_ragged(fr, tt, b, 0.1)
        bkeys = batch.sigma1_map_ragged(fr, b)
        bext = batch.extract_keyed_ragged(wm, bkeys, b, 0.1)
        n = len(specs)
        for order in (list(range(n))[::-1], [int(k) for k in np.random.default_rng(5).permutation(n)]):
            keys = batch.sigma1_map_ragged([fr[k] for k in order], b)
            ext = batch.extract_keyed_ragged([wm[k] for k in order], keys, b, 0.1)
            for pos, k in enumerate(order):
                assert _same_bits(keys[pos], bkeys[k]), (b, order, pos)
                assert torch.equal(ext[pos], bext[k]), (b, order, pos)


def test_shared_keys(dev):
    """One 139 x 203 original, three watermarked copies with different tiles and the same key
    tensor three times, next to a 64 x 96 frame with its own key."""
    from thatsmyface_amd import batch

    b = 8
    specs = [("photo", 139, 203, 0)] * 3 + [("noise", 64, 96, 1)]
    covers, tiles = _frames(specs, b, 1400)
    fr, tt = _dev(covers, dev), _dev(tiles, dev)
    wm = batch.embed_ragged(fr, tt, b, 0.1)
    k0, k3 = batch.sigma1_map_ragged([fr[0], fr[3]], b)
    ext = batch.extract_keyed_ragged(wm, [k0, k0, k0, k3], b, 0.1)
    pair = batch.extract_ragged(wm, fr, b, 0.1)
    for i in range(4):
        assert torch.equal(ext[i], pair[i]), i
        assert torch.equal(ext[i], batch.extract_batch(wm[i][None], fr[i][None], b, 0.1)[0]), i
    assert not torch.equal(ext[0], ext[1]) and not torch.equal(ext[1], ext[2])  # three tiles


@pytest.mark.parametrize("b", ALL_B)
def test_dgesdd_route_taken_on_the_hybrid_route(dev, b):
    """Sparks frames (keyed_helpers.sparks) of three sizes: the enclosure decides no block of
    them, so each goes from the strip pass straight to the dgesdd route; a fourth frame's first
    17 block columns are noise, the rest sparks.  lapack_blocks must be the exact count of
    sparks blocks: no noise block reaches the dgesdd route although no list pass runs."""
    from golden.gen_golden import wmark

    from thatsmyface_amd import batch

    shapes = [(3 * b + 3, 35 * b + 5), (4 * b, 64 * b), (b, b)]
    covers = [sparks(H, W, b, 40 + i) for i, (H, W) in enumerate(shapes)]
    half = sparks(*shapes[0], b, 50)
    half[:, : 17 * b] = _u8(51, (shapes[0][0], 17 * b, 3))
    covers.append(half)
    # the sparks blocks: every block of the three frames, the block columns from 17 on of the fourth
    # (W // b of them in all: 36 at b = 4, where 35 b + 5 holds one more block, 35 otherwise)
    expect = sum((H // b) * (W // b) for H, W in shapes) + (shapes[0][0] // b) * (shapes[0][1] // b - 17)
    tiles = [wmark("noise", c.shape[0] // b, c.shape[1] // b, 4 + i) for i, c in enumerate(covers)]
    fr, tt = _dev(covers, dev), _dev(tiles, dev)
    wm = batch.embed_ragged(fr, tt, b, 0.1)
    sm, sx = {}, {}
    keys = batch.sigma1_map_ragged(fr, b, stats=sm)
    ext = batch.extract_keyed_ragged(wm, keys, b, 0.1, stats=sx)
    print("dgesdd-route blocks", b, sm, sx, "sparks blocks", expect)
    for i, c in enumerate(covers):
        assert np.array_equal(_bits(keys[i]), _bits(key_of(c, b))), (b, i)
        assert np.array_equal(ext[i].cpu().numpy(), O.extract_frame(wm[i].cpu().numpy(), c, b, 0.1, route="lapack")), (b, i)
    assert sm == {"lapack_blocks": expect, "list_pass_blocks": 0} and sx == sm, (sm, sx, expect)


def test_chunks(dev, monkeypatch):
    """TMFWM_DEBUG_LIST_CAP below any two frames' blocks: every frame is a chunk of its own, and
    each chunk's frame table slice, lists and counts must be its own."""
    from golden.gen_golden import cover

    from thatsmyface_amd import batch

    b = 8
    covers = [np.ascontiguousarray(cover("smooth", 64, 128, 30)), sparks(48, 136, b, 31), np.ascontiguousarray(cover("qr", 72, 96, 32)),
              sparks(64, 120, b, 33)]
    nbs = [(c.shape[0] // b) * (c.shape[1] // b) for c in covers]
    tiles = [_u8(34 + i, (c.shape[0] // b, c.shape[1] // b)) for i, c in enumerate(covers)]
    fr, tt = _dev(covers, dev), _dev(tiles, dev)
    wm = batch.embed_ragged(fr, tt, b, 0.1)

    def run():
        sm, sx = {}, {}
        keys = batch.sigma1_map_ragged(fr, b, stats=sm)
        return keys, batch.extract_keyed_ragged(wm, keys, b, 0.1, stats=sx), sm, sx

    k0, x0, sm0, sx0 = run()
    cap = max(nbs) + 1
    assert all(x + y > cap for i, x in enumerate(nbs) for y in nbs[i + 1:])  # no two frames share a chunk
    monkeypatch.setenv("TMFWM_DEBUG_LIST_CAP", str(cap))
    k1, x1, sm1, sx1 = run()
    assert sm1 == sm0 and sx1 == sx0 and sm0["lapack_blocks"] >= nbs[1] + nbs[3] and sx0["lapack_blocks"] >= nbs[1] + nbs[3], (sm0, sm1, sx0, sx1)
    pair = batch.extract_ragged(wm, fr, b, 0.1)
    for i in range(4):
        assert _same_bits(k1[i], k0[i]) and torch.equal(x1[i], x0[i]) and torch.equal(x1[i], pair[i]), i


def test_malformed_and_negative_key_entries(dev):
    """As test_keyed_gpu's: non-finite key entries give byte 0; a finite entry, -1.0 included,
    gives extract_byte's value; the other blocks are untouched -- on two frames of two sizes."""
    from thatsmyface_amd import batch

    b = 8
    covers = [_u8(60, (40, 72, 3)), _u8(62, (56, 88, 3))]
    tiles = [_u8(61 + i, (c.shape[0] // b, c.shape[1] // b)) for i, c in enumerate(covers)]
    fr, tt = _dev(covers, dev), _dev(tiles, dev)
    wm = batch.embed_ragged(fr, tt, b, 0.1)
    keys = batch.sigma1_map_ragged(fr, b)
    kw = [k.cpu().numpy() for k in batch.sigma1_map_ragged(wm, b)]
    bad = [k.clone() for k in keys]
    bad[0][0, 0], bad[0][1, 2], bad[1][2, 3], bad[1][4, 8], bad[0][3, 3] = float("nan"), float("inf"), float("-inf"), -1.0, 3.0e38
    zero = {0: ((0, 0), (1, 2)), 1: ((2, 3),)}
    for route in ("hybrid", "reference"):
        for alpha in (0.1, -0.5):
            got = [g.cpu().numpy() for g in batch.extract_keyed_ragged(wm, bad, b, alpha, route=route)]
            for f in range(2):
                exp = bytes_of(kw[f], np.nan_to_num(bad[f].cpu().numpy(), nan=0.0, posinf=0.0, neginf=0.0), alpha)
                for at in zero[f]:
                    exp[at] = 0
                assert np.array_equal(got[f], exp), (route, alpha, f)
            assert got[1][4, 8] == (255 if alpha > 0 else 0) and got[0][3, 3] == (0 if alpha > 0 else 255)
    for f in range(2):  # sanity of the expectation itself: with the sound key it is the pair path
        assert np.array_equal(bytes_of(kw[f], keys[f].cpu().numpy(), 0.1), batch.extract_batch(wm[f][None], fr[f][None], b, 0.1)[0].cpu().numpy())


def test_ctypes_memory_kinds_overlap_and_pointers(dev):
    from thatsmyface_amd import _lib, batch

    L = _lib.load()
    b = 8
    specs = [("qr", 40, 64, 0), ("diagonal", 139, 203, 0), ("blocky", 37, 61, 0), ("noise", 5, 9, 0)]
    covers, tiles = _frames(specs, b, 1000)
    n = len(specs)
    fr, tt = _dev(covers, dev), _dev(tiles, dev)
    wm = batch.embed_ragged(fr, tt, b, 0.1)
    sm, sx = {}, {}
    keys = batch.sigma1_map_ragged(fr, b, stats=sm)
    ext = batch.extract_keyed_ragged(wm, keys, b, 0.1, stats=sx)
    assert sm["lapack_blocks"] > 0 and sx["lapack_blocks"] > 0  # the counts are real sums
    # host memory gives the device-memory bits
    wm_h = [w.cpu().numpy() for w in wm]
    hk = [np.full(k.shape, -3.0, np.float32) for k in keys]
    cnt = ctypes.c_int64(-1)
    md = _desc(_lib.KeyFrame, [(c.ctypes.data, k.ctypes.data if k.size else None, c.shape[0], c.shape[1]) for c, k in zip(covers, hk)])
    _lib.check(L.tmfwm_sigma1_map_ragged(ctypes.addressof(md), n, b, _lib.MEM_HOST, None, 0, ctypes.addressof(cnt)), "map")
    assert cnt.value == sm["lapack_blocks"] and L.tmfwm_last_list_pass_blocks() == 0
    ht = [np.full(t.shape, 7, np.uint8) for t in tiles]
    cnt = ctypes.c_int64(-1)
    kd = _desc(_lib.KeyedFrame, [(w.ctypes.data, k.ctypes.data if k.size else None, t.ctypes.data if t.size else None, w.shape[0], w.shape[1])
                                 for w, k, t in zip(wm_h, hk, ht)])
    _lib.check(L.tmfwm_extract_keyed_ragged(ctypes.addressof(kd), n, b, 0.1, _lib.MEM_HOST, None, 0, ctypes.addressof(cnt)), "keyed")
    assert cnt.value == sx["lapack_blocks"]
    for i in range(n):
        assert np.array_equal(_bits(hk[i]), _bits(keys[i])), i
        assert np.array_equal(ht[i], ext[i].cpu().numpy()), i
    # the asynchronous form (no count pointer) into caller buffers
    stream = torch.cuda.current_stream().cuda_stream
    dk = [torch.full(k.shape, -3.0, dtype=torch.float32, device=dev) for k in keys]
    dt = [torch.full(t.shape, 9, dtype=torch.uint8, device=dev) for t in ext]
    md = _desc(_lib.KeyFrame, [(f.data_ptr(), k.data_ptr() if k.numel() else None, f.shape[0], f.shape[1]) for f, k in zip(fr, dk)])
    _lib.check(L.tmfwm_sigma1_map_ragged(ctypes.addressof(md), n, b, _lib.MEM_DEVICE, stream, 0, None), "map")
    ctypes.memset(ctypes.addressof(md), 0xA5, ctypes.sizeof(md))  # the call has returned: the array is the caller's again
    krows = [(w.data_ptr(), k.data_ptr() if k.numel() else None, t.data_ptr() if t.numel() else None, w.shape[0], w.shape[1])
             for w, k, t in zip(wm, dk, dt)]
    kd = _desc(_lib.KeyedFrame, krows)
    _lib.check(L.tmfwm_extract_keyed_ragged(ctypes.addressof(kd), n, b, 0.1, _lib.MEM_DEVICE, stream, 0, None), "keyed")
    ctypes.memset(ctypes.addressof(kd), 0x5A, ctypes.sizeof(kd))
    torch.cuda.synchronize()
    for i in range(n):
        assert _same_bits(dk[i], keys[i]) and torch.equal(dt[i], ext[i]), i

    def refused(kind, rows, match="overlaps"):
        d = _desc(kind, rows)
        if kind is _lib.KeyFrame:
            rc = L.tmfwm_sigma1_map_ragged(ctypes.addressof(d), len(rows), b, _lib.MEM_DEVICE, stream, 0, None)
        else:
            rc = L.tmfwm_extract_keyed_ragged(ctypes.addressof(d), len(rows), b, 0.1, _lib.MEM_DEVICE, stream, 0, None)
        assert rc == _lib.ERR_INVALID and match in _lib.last_error(), (rc, _lib.last_error())

    # an out_tile inside a wm_rgb (another frame's), an out_tile inside a key, an out_key inside another frame's out_key
    bad = list(krows)
    bad[0] = (krows[0][0], krows[0][1], wm[1].data_ptr() + 5, 40, 64)
    refused(_lib.KeyedFrame, bad)
    bad[0] = (krows[0][0], krows[0][1], dk[1].data_ptr() + 8, 40, 64)
    refused(_lib.KeyedFrame, bad)
    mrows = [(f.data_ptr(), k.data_ptr() if k.numel() else None, f.shape[0], f.shape[1]) for f, k in zip(fr, dk)]
    mbad = list(mrows)
    mbad[2] = (mrows[2][0], dk[1].data_ptr() + 16, 37, 61)
    refused(_lib.KeyFrame, mbad)
    mbad[2] = (mrows[2][0], fr[2].data_ptr() + 4, 37, 61)  # an out_key inside its own input
    refused(_lib.KeyFrame, mbad)
    # inputs may share memory: one key for two frames of its size is no overlap
    two = [krows[0], (wm[0].data_ptr(), krows[0][1], dt[1].data_ptr(), 40, 64)]
    d = _desc(_lib.KeyedFrame, two)
    _lib.check(L.tmfwm_extract_keyed_ragged(ctypes.addressof(d), 2, b, 0.1, _lib.MEM_DEVICE, stream, 0, None), "shared key")
    torch.cuda.synchronize()
    assert torch.equal(dt[1].view(-1)[: ext[0].numel()].view(ext[0].shape), ext[0])
    # a host pointer passed as device memory is refused and never dereferenced
    hkey = np.zeros((5, 8), np.float32)
    refused(_lib.KeyedFrame, [(wm[0].data_ptr(), hkey.ctypes.data, dt[0].data_ptr(), 40, 64)], match="not")
    refused(_lib.KeyFrame, [(fr[0].data_ptr(), hkey.ctypes.data, 40, 64)], match="not")
    refused(_lib.KeyFrame, [(covers[0].ctypes.data, dk[0].data_ptr(), 40, 64)], match="not")
    # the Python layer's own checks
    with pytest.raises(TypeError, match="float32"):
        batch.extract_keyed_ragged(wm, [k.double() for k in keys], b, 0.1)
    with pytest.raises(ValueError, match="one block size and one image size"):
        batch.extract_keyed_ragged(wm, keys[1:] + keys[:1], b, 0.1)
    with pytest.raises(ValueError, match="contiguous"):
        batch.extract_keyed_ragged(wm[:1], [torch.zeros((8, 5), dtype=torch.float32, device=dev).t()], b, 0.1)
    with pytest.raises(ValueError, match="keys"):
        batch.extract_keyed_ragged(wm, keys[:-1], b, 0.1)
    with pytest.raises(ValueError, match="out"):
        batch.sigma1_map_ragged(fr, b, out=[torch.empty_like(k) for k in keys[:-1]])
    with pytest.raises(ValueError, match="out"):
        batch.extract_keyed_ragged(wm, keys, b, 0.1, out=[torch.empty_like(k) for k in keys])  # float tiles
    given = [torch.empty_like(t) for t in ext]
    got = batch.extract_keyed_ragged(wm, keys, b, 0.1, out=given)
    assert all(g is o for g, o in zip(got, given)) and all(torch.equal(g, e) for g, e in zip(got, ext))
    kgiven = [torch.empty_like(k) for k in keys]
    kgot = batch.sigma1_map_ragged(fr, b, out=kgiven)
    assert all(g is o for g, o in zip(kgot, kgiven)) and all(_same_bits(g, k) for g, k in zip(kgot, keys))


def test_nonconvergence_fails_a_synchronising_call(dev, monkeypatch):
    from thatsmyface_amd import _lib, batch

    fr = _dev([_u8(1100, (40, 64, 3)), _u8(1101, (24, 16, 3))], dev)
    keys = batch.sigma1_map_ragged(fr, 8)
    monkeypatch.setenv("TMFWM_DEBUG_FORCE_NONCONV", "1")
    with pytest.raises(_lib.TmfwmError, match="did not converge"):
        batch.sigma1_map_ragged(fr, 8, stats={})
    with pytest.raises(_lib.TmfwmError, match="did not converge"):
        batch.extract_keyed_ragged(fr, keys, 8, 0.1, stats={})
    # the asynchronous call does not look at the count
    batch.sigma1_map_ragged(fr, 8)
    batch.extract_keyed_ragged(fr, keys, 8, 0.1)
    torch.cuda.synchronize()


def test_pipeline_extracts_images(dev, golden_alpha):
    """extract_images over six PNGs of three sizes in groups of four gives the bytes of
    extract_watermark_keyed per image; on one golden fixture per block size, the fixture's."""
    from thatsmyface_amd import pipeline
    from thatsmyface_amd import watermarking as W

    settings = {"block_size": 8, "alpha": 0.15}
    sizes = [(96, 128), (120, 90), (96, 128), (64, 200), (120, 90), (64, 200)]
    origs = [Image.fromarray(_cover("photo" if i % 2 else "noise", h, w, 1200 + i)) for i, (h, w) in enumerate(sizes)]
    wms = [Image.fromarray((_u8(1300 + i, (29, 29)) & 1) * 255, "L") for i in range(6)]
    embedded = pipeline.embed_images(origs, wms, True, settings, batch_images=4)
    keys = [W.extraction_key(o, settings) for o in origs]
    imgs = [e.png if i % 3 else e.image() for i, e in enumerate(embedded)]
    got = list(pipeline.extract_images(imgs, keys, settings, batch_images=4))
    assert len(got) == 6
    for i, g in enumerate(got):
        want = W.extract_watermark_keyed(embedded[i].image(), keys[i], settings)
        assert g.mode == "L" and g.size == want.size and np.array_equal(np.asarray(g), np.asarray(want)), i
    assert not np.array_equal(np.asarray(got[0]), np.asarray(got[2]))  # one size, two watermarks
    # a shared key array: one original, two watermarked copies, next to an image smaller than a block
    twice = pipeline.embed_images([origs[0], origs[0]], wms[:2], True, settings, batch_images=2)
    tiny = Image.fromarray(_u8(5, (5, 30, 3)))
    with pytest.raises(ValueError, match="one block size and one image size"):
        list(pipeline.extract_images([twice[0].image()], [keys[1]], settings, batch_images=4))
    got2 = list(pipeline.extract_images([twice[0].png, twice[1].png], [keys[0], keys[0]], settings, batch_images=4))
    for e, g in zip(twice, got2):
        assert np.array_equal(np.asarray(g), np.asarray(W.extract_watermark(e.image(), origs[0], settings)))
    del tiny
    # one golden fixture per block size, all of them in one call per block size's settings
    cases, meta = golden_alpha
    seen = set()
    for name, m in meta["cases"].items():
        if m["block"] in seen:
            continue
        seen.add(m["block"])
        arr = cases[f"{name}/cover"]
        cov = Image.fromarray(arr, "L" if arr.ndim == 2 else ("RGBA" if arr.shape[-1] == 4 else "RGB"))
        s = {"block_size": m["block"], "alpha": m["alpha"]}
        emb = Image.fromarray(cases[f"{name}/embed"])
        (ex,) = pipeline.extract_images([emb], [W.extraction_key(cov, s)], s, batch_images=4)
        assert ex.mode == "L" and np.array_equal(np.asarray(ex), cases[f"{name}/extract"]), name
    assert seen == set(ALL_B)
