"""Ragged batches on the GPU: batch.embed_ragged / extract_ragged, tmfwm_embed_ragged /
tmfwm_extract_ragged through ctypes, pipeline.embed_images(batch_images=K).

Every frame of a ragged call has two yardsticks: the oracle's single-frame result, and the
single-size path (batch.embed_batch / extract_batch, unchanged code) called on that frame alone,
which also covers the shapes the oracle is not asked about (a frame without a full block).
"""
import ctypes
import io

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ALL_B = (4, 6, 8, 10, 12, 14, 16)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from thatsmyface_amd import _lib

    assert _lib.device_count() > 0
    return torch.device("cuda", 0)


def _u8(seed, shape):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def _cover(kind, H, W, seed):
    from golden.gen_golden import cover
    from lapack_path import photo_cover

    return photo_cover(H, W, seed) if kind == "photo" else np.ascontiguousarray(cover(kind, H, W, seed))


def _tile(i, nbh, nbw, seed):
    """Uniform bytes and binary 0 / 255 (QR-like) tiles alternate."""
    from golden.gen_golden import wmark

    return _u8(seed + i, (nbh, nbw)) if i % 2 == 0 else wmark("qr", nbh, nbw, seed + i)


def _frames(specs, b, seed):
    """specs: (kind, H, W, cover seed offset) per frame -> (covers, tiles); equal (kind, H, W, offset) give one cover."""
    made = {}
    covers, tiles = [], []
    for i, (kind, H, W, off) in enumerate(specs):
        key = (kind, H, W, off)
        if key not in made:
            made[key] = _cover(kind, H, W, seed + off)
        covers.append(made[key])
        tiles.append(_tile(i, H // b, W // b, seed + 100))
    return covers, tiles


def _dev(arrays, dev):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def _single(batch, fr, tt, b, alpha, route="hybrid"):
    """The single-size path on every frame alone: (outputs, extracted tiles, summed lapack_blocks of embed)."""
    outs, exts, total = [], [], 0
    for f, t in zip(fr, tt):
        st = {}
        o = batch.embed_batch(f[None], t, b, alpha, stats=st, route=route)
        total += st["lapack_blocks"]
        outs.append(o[0])
        exts.append(batch.extract_batch(o, f[None], b, alpha, route=route)[0])
    return outs, exts, total


def _mixed_specs(b):
    return [("noise", 139, 203, 0), ("diagonal", 139, 203, 0), ("photo", 139, 203, 0), ("noise", 139, 203, 0),  # 0 / 3: one cover, two tiles
            ("smooth", 203, 139, 0), ("qr", 203, 139, 0),  # one size, two covers
            ("noise", b, b, 1), ("noise", b - 1, 50, 2), ("blocky", 37, 61, 0), ("smooth", 64, 256, 0)]


@pytest.mark.parametrize("b", ALL_B)
def test_every_slider_size_hybrid_mixed_shapes(dev, b):
    """One call over frames of 139 x 203 (three kinds that reach the dgesdd route at every b, and
    a twin of the first with another tile), 203 x 139 twice, b x b (one block), (b-1) x 50 (no
    block: all edge), 37 x 61 (W % 4 != 0: byte loads next to aligned frames) and 64 x 256."""
    from thatsmyface_amd import batch

    specs = _mixed_specs(b)
    covers, tiles = _frames(specs, b, 900 + b)
    fr, tt = _dev(covers, dev), _dev(tiles, dev)
    st = {}
    out = batch.embed_ragged(fr, tt, b, 0.1, stats=st)
    print("stats", b, st)
    assert st["lapack_blocks"] > 0 and st["list_pass_blocks"] == 0, st
    sx = {}
    ext = batch.extract_ragged(out, fr, b, 0.1, stats=sx)
    souts, sexts, stotal = _single(batch, fr, tt, b, 0.1)
    assert st["lapack_blocks"] == stotal, (st, stotal)
    assert len({o.data_ptr() for o in out}) == len(out)
    for i, (kind, H, W, _) in enumerate(specs):
        assert out[i].shape == (H, W, 3) and ext[i].shape == (H // b, W // b)
        assert torch.equal(out[i], souts[i]), (b, i)
        assert torch.equal(ext[i], sexts[i]), (b, i)
        if H >= b and W >= b:
            ref = O.embed_frame(covers[i], tiles[i], b, 0.1)
            assert np.array_equal(out[i].cpu().numpy(), ref), (b, i)
            assert np.array_equal(ext[i].cpu().numpy(), O.extract_frame(ref, covers[i], b, 0.1)), (b, i)
    assert not torch.equal(out[0], out[3]) and not torch.equal(out[4], out[5])  # the twins differ


def test_position_independence(dev):
    from thatsmyface_amd import batch

    for b in (8, 14):
        specs = _mixed_specs(b)
        covers, tiles = _frames(specs, b, 940 + b)
        fr, tt = _dev(covers, dev), _dev(tiles, dev)
        base = batch.embed_ragged(fr, tt, b, 0.1)
        bext = batch.extract_ragged(base, fr, b, 0.1)
        n = len(specs)
        for order in (list(range(n))[::-1], [int(k) for k in np.random.default_rng(5).permutation(n)]):
            out = batch.embed_ragged([fr[k] for k in order], [tt[k] for k in order], b, 0.1)
            ext = batch.extract_ragged(out, [fr[k] for k in order], b, 0.1)
            for pos, k in enumerate(order):
                assert torch.equal(out[pos], base[k]), (b, order, pos)
                assert torch.equal(ext[pos], bext[k]), (b, order, pos)


@pytest.mark.parametrize("b", ALL_B)
def test_reference_route(dev, b):
    """The reference route against the oracle's dgesdd route on four frames; at b = 8 and 16 the
    ragged hybrid bytes equal the ragged reference bytes; at b = 8 a large and a negative alpha."""
    from thatsmyface_amd import batch

    specs = [("noise", 139, 203, 0), ("photo", 64, 96, 0), ("noise", 139, 203, 0), ("blocky", 37, 61, 0)]
    covers, tiles = _frames(specs, b, 960 + b)
    fr, tt = _dev(covers, dev), _dev(tiles, dev)
    nblocks = sum((H // b) * (W // b) for _, H, W, _ in specs)
    st = {}
    ref = batch.embed_ragged(fr, tt, b, 0.1, route="reference", stats=st)
    assert st["lapack_blocks"] == nblocks, st
    sx = {}
    ext = batch.extract_ragged(ref, fr, b, 0.1, route="reference", stats=sx)
    assert sx["lapack_blocks"] == nblocks, sx
    for i in range(len(specs)):
        want = O.embed_frame(covers[i], tiles[i], b, 0.1, route="lapack")
        assert np.array_equal(ref[i].cpu().numpy(), want), (b, i)
        assert np.array_equal(ext[i].cpu().numpy(), O.extract_frame(want, covers[i], b, 0.1, route="lapack")), (b, i)
    assert not torch.equal(ref[0], ref[2])
    if b in (8, 16):
        hyb = batch.embed_ragged(fr, tt, b, 0.1, route="hybrid")
        for i in range(len(specs)):
            assert torch.equal(hyb[i], ref[i]), (b, i)
    if b == 8:
        for alpha in (1.0, -5.0):
            ref_a = batch.embed_ragged(fr, tt, b, alpha, route="reference")
            hyb_a = batch.embed_ragged(fr, tt, b, alpha, route="hybrid")
            for i in range(len(specs)):
                assert torch.equal(hyb_a[i], ref_a[i]), (alpha, i)
            assert np.array_equal(ref_a[1].cpu().numpy(), O.embed_frame(covers[1], tiles[1], b, alpha, route="lapack")), alpha


def test_many_tiny_frames(dev):
    """300 frames cycling through 8 x 8, 9 x 17, 24 x 16, 16 x 40 and 7 x 7 at b = 8: the binary
    searches cross hundreds of boundaries and every fifth frame has no wave and no block."""
    from thatsmyface_amd import batch

    b, sizes = 8, [(8, 8), (9, 17), (24, 16), (16, 40), (7, 7)]
    covers = [_u8(3000 + i, (*sizes[i % 5], 3)) for i in range(300)]
    tiles = [_u8(4000 + i, (sizes[i % 5][0] // b, sizes[i % 5][1] // b)) for i in range(300)]
    fr, tt = _dev(covers, dev), _dev(tiles, dev)
    souts, sexts, stotal = _single(batch, fr, tt, b, 0.1)
    for route in ("hybrid", "reference"):
        st = {}
        out = batch.embed_ragged(fr, tt, b, 0.1, stats=st, route=route)
        ext = batch.extract_ragged(out, fr, b, 0.1, route=route)
        if route == "hybrid":
            assert st["lapack_blocks"] == stotal, (st, stotal)
        for i in range(300):
            assert torch.equal(out[i], souts[i]), (route, i)
            assert torch.equal(ext[i], sexts[i]), (route, i)
    # one frame, and one frame without a block
    for i in (3, 4):
        one = batch.embed_ragged(fr[i:i + 1], tt[i:i + 1], b, 0.1)
        assert len(one) == 1 and torch.equal(one[0], souts[i])
        xone = batch.extract_ragged(one, fr[i:i + 1], b, 0.1)
        assert len(xone) == 1 and torch.equal(xone[0], sexts[i])
    assert batch.embed_ragged([], [], b, 0.1) == [] and batch.extract_ragged([], [], b, 0.1) == []


def test_chunks(dev, monkeypatch):
    """TMFWM_DEBUG_LIST_CAP bounds a ragged chunk: 2500 ids cut 2040 + 425 | 2040 + 256 blocks,
    2100 ids put every frame in a chunk of its own; bytes and counts equal the unchunked call."""
    from thatsmyface_amd import batch

    b = 8
    specs = [("smooth", 272, 480, 0), ("noise", 136, 200, 0), ("qr", 272, 480, 0), ("blocky", 64, 256, 0)]
    covers, tiles = _frames(specs, b, 70)
    fr, tt = _dev(covers, dev), _dev(tiles, dev)
    st0, sx0 = {}, {}
    out0 = batch.embed_ragged(fr, tt, b, 0.1, stats=st0)
    ext0 = batch.extract_ragged(out0, fr, b, 0.1, stats=sx0)
    ref0 = batch.embed_ragged(fr, tt, b, 0.1, route="reference")
    assert st0["lapack_blocks"] > 0, st0
    for i in range(len(specs)):
        assert np.array_equal(out0[i].cpu().numpy(), O.embed_frame(covers[i], tiles[i], b, 0.1)), i
    for cap in (2500, 2100):
        monkeypatch.setenv("TMFWM_DEBUG_LIST_CAP", str(cap))
        st1, sx1 = {}, {}
        out1 = batch.embed_ragged(fr, tt, b, 0.1, stats=st1)
        ext1 = batch.extract_ragged(out1, fr, b, 0.1, stats=sx1)
        ref1 = batch.embed_ragged(fr, tt, b, 0.1, route="reference")
        assert st1 == st0 and sx1 == sx0, (cap, st0, st1, sx0, sx1)
        for i in range(len(specs)):
            assert torch.equal(out1[i], out0[i]) and torch.equal(ext1[i], ext0[i]) and torch.equal(ref1[i], ref0[i]), (cap, i)


def _desc(kind, rows):
    d = (kind * len(rows))()
    for i, r in enumerate(rows):
        d[i] = kind(*r)
    return d


def test_ctypes_host_and_misaligned_device(dev):
    from thatsmyface_amd import _lib, batch

    L = _lib.load()
    b = 8
    # diagonal and qr covers: blocks for the dgesdd route, so the count is a real sum
    specs = [("qr", 40, 64, 0), ("diagonal", 139, 203, 0), ("qr", 40, 64, 0), ("blocky", 37, 61, 0), ("noise", 5, 9, 0)]
    covers, tiles = _frames(specs, b, 1000)
    n = len(specs)
    fr, tt = _dev(covers, dev), _dev(tiles, dev)
    souts, sexts, stotal = _single(batch, fr, tt, b, 0.1)
    assert stotal > 0
    # host memory
    outs = [np.zeros_like(c) for c in covers]
    cnt = ctypes.c_int64(-1)
    ed = _desc(_lib.EmbedFrame, [(c.ctypes.data, o.ctypes.data, t.ctypes.data if t.size else None, c.shape[0], c.shape[1])
                                 for c, o, t in zip(covers, outs, tiles)])
    _lib.check(L.tmfwm_embed_ragged(ctypes.addressof(ed), n, b, 0.1, _lib.MEM_HOST, None, 0, ctypes.addressof(cnt)), "embed_ragged")
    assert cnt.value == stotal and L.tmfwm_last_list_pass_blocks() == 0
    xts = [np.full(t.shape, 7, np.uint8) for t in tiles]
    xd = _desc(_lib.ExtractFrame, [(o.ctypes.data, c.ctypes.data, x.ctypes.data if x.size else None, c.shape[0], c.shape[1])
                                   for c, o, x in zip(covers, outs, xts)])
    _lib.check(L.tmfwm_extract_ragged(ctypes.addressof(xd), n, b, 0.1, _lib.MEM_HOST, None, 0, None), "extract_ragged")
    for i in range(n):
        assert np.array_equal(outs[i], souts[i].cpu().numpy()), i
        assert np.array_equal(xts[i], sexts[i].cpu().numpy()), i
    # device frames at odd and even byte offsets in one buffer: aligned for some frames, not for others
    sizes = [c.size for c in covers]
    pad = [0, 1, 4, 3, 2]  # bytes skipped before each frame: offsets 0, odd, multiple of 4, ...
    total = sum(s + 8 for s in sizes) + 16
    big_in = torch.zeros(total, dtype=torch.uint8, device=dev)
    big_out = torch.zeros(total, dtype=torch.uint8, device=dev)
    offs, o = [], 0
    for s, p in zip(sizes, pad):
        o = (o + 3) // 4 * 4 + p
        offs.append(o)
        o += s
    assert {x % 4 for x in offs} == {0, 1, 2, 3}
    vin = [big_in[o:o + s].view(c.shape) for o, s, c in zip(offs, sizes, covers)]
    vout = [big_out[o:o + s].view(c.shape) for o, s, c in zip(offs, sizes, covers)]
    for v, f in zip(vin, fr):
        v.copy_(f)
    torch.cuda.synchronize()
    rows = [(v.data_ptr(), w.data_ptr(), t.data_ptr() if t.numel() else None, v.shape[0], v.shape[1]) for v, w, t in zip(vin, vout, tt)]
    ed = _desc(_lib.EmbedFrame, rows)
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(L.tmfwm_embed_ragged(ctypes.addressof(ed), n, b, 0.1, _lib.MEM_DEVICE, stream, 0, None), "embed_ragged")
    ctypes.memset(ctypes.addressof(ed), 0xA5, ctypes.sizeof(ed))  # the asynchronous call has returned: the array is the caller's again
    del ed
    xout = [torch.full(t.shape, 9, dtype=torch.uint8, device=dev) for t in tt]
    xd = _desc(_lib.ExtractFrame, [(w.data_ptr(), v.data_ptr(), x.data_ptr() if x.numel() else None, v.shape[0], v.shape[1])
                                   for v, w, x in zip(vin, vout, xout)])
    _lib.check(L.tmfwm_extract_ragged(ctypes.addressof(xd), n, b, 0.1, _lib.MEM_DEVICE, stream, 0, None), "extract_ragged")
    ctypes.memset(ctypes.addressof(xd), 0x5A, ctypes.sizeof(xd))
    del xd
    torch.cuda.synchronize()
    for i in range(n):
        assert torch.equal(vout[i], souts[i]), i
        assert torch.equal(xout[i], sexts[i]), i
    written = torch.zeros(total, dtype=torch.bool, device=dev)
    for o, s in zip(offs, sizes):
        written[o:o + s] = True
    assert not big_out[~written].any()  # nothing outside the frames
    # an output inside another frame's input, and two outputs that share bytes
    bad = list(rows)
    bad[2] = (rows[2][0], rows[0][0] + 5, rows[2][2], rows[2][3], rows[2][4])
    bd = _desc(_lib.EmbedFrame, bad)
    with pytest.raises(ValueError, match="overlaps"):
        _lib.check(L.tmfwm_embed_ragged(ctypes.addressof(bd), n, b, 0.1, _lib.MEM_DEVICE, stream, 0, None), "e")
    bad[2] = (rows[2][0], rows[1][1] + 12, rows[2][2], rows[2][3], rows[2][4])
    bd = _desc(_lib.EmbedFrame, bad)
    with pytest.raises(ValueError, match="overlaps"):
        _lib.check(L.tmfwm_embed_ragged(ctypes.addressof(bd), n, b, 0.1, _lib.MEM_DEVICE, stream, 0, None), "e")
    xbad = _desc(_lib.ExtractFrame, [(vout[0].data_ptr(), vin[0].data_ptr(), vin[0].data_ptr() + 3, 40, 64)])
    with pytest.raises(ValueError, match="overlaps"):
        _lib.check(L.tmfwm_extract_ragged(ctypes.addressof(xbad), 1, b, 0.1, _lib.MEM_DEVICE, stream, 0, None), "x")
    with pytest.raises(ValueError, match="not"):  # a host pointer handed in as device memory
        hd = _desc(_lib.EmbedFrame, [(covers[0].ctypes.data, vout[0].data_ptr(), tt[0].data_ptr(), 40, 64)])
        _lib.check(L.tmfwm_embed_ragged(ctypes.addressof(hd), 1, b, 0.1, _lib.MEM_DEVICE, stream, 0, None), "e")
    ok = _desc(_lib.EmbedFrame, rows)
    for route in (_lib.ROUTE_RANK1, _lib.ROUTE_RANK1_REFERENCE):
        assert L.tmfwm_embed_ragged(ctypes.addressof(ok), n, b, 0.1, _lib.MEM_DEVICE, stream, route, None) == _lib.ERR_UNSUPPORTED
        assert "rank-1" in _lib.last_error()
    # the Python layer's own checks
    with pytest.raises(ValueError, match="tiles"):
        batch.embed_ragged(fr, tt[:-1], b, 0.1)
    with pytest.raises(ValueError, match="tiles"):
        batch.embed_ragged(fr, tt[1:] + tt[:1], b, 0.1)
    with pytest.raises(ValueError, match="frames"):
        batch.embed_ragged([f.cpu() for f in fr], tt, b, 0.1)
    with pytest.raises(ValueError, match="frames"):
        batch.embed_ragged([f.to(torch.int16) for f in fr], tt, b, 0.1)
    with pytest.raises(ValueError, match="shapes differ"):
        batch.extract_ragged(fr, fr[1:] + fr[:1], b, 0.1)
    with pytest.raises(ValueError, match="out"):
        batch.embed_ragged(fr, tt, b, 0.1, out=[torch.empty_like(f) for f in fr[:-1]])
    given = [torch.empty_like(f) for f in fr]
    got = batch.embed_ragged(fr, tt, b, 0.1, out=given)
    assert all(g is o for g, o in zip(got, given)) and all(torch.equal(g, s) for g, s in zip(got, souts))


def test_nonconvergence_fails_a_synchronising_call(dev, monkeypatch):
    from thatsmyface_amd import _lib, batch

    covers, tiles = _frames([("noise", 40, 64, 0), ("noise", 24, 16, 0)], 8, 1100)
    fr, tt = _dev(covers, dev), _dev(tiles, dev)
    monkeypatch.setenv("TMFWM_DEBUG_FORCE_NONCONV", "1")
    with pytest.raises(_lib.TmfwmError, match="did not converge"):
        batch.embed_ragged(fr, tt, 8, 0.1, stats={})
    with pytest.raises(_lib.TmfwmError, match="did not converge"):
        batch.extract_ragged(fr, fr, 8, 0.1, stats={})


def test_pipeline_batches_images(dev):
    """embed_images over six images of four sizes with six watermarks: groups of four (one full,
    one short) give the pixels and PNG bytes of the per-image path, in order."""
    from PIL import Image

    from thatsmyface_amd import pipeline

    sizes = [(96, 128), (120, 90), (96, 128), (64, 200), (75, 75), (120, 90)]
    imgs, wms = [], []
    for i, (h, w) in enumerate(sizes):
        arr = _cover("photo" if i % 2 else "noise", h, w, 1200 + i)
        buf = io.BytesIO()
        Image.fromarray(arr).save(buf, format="PNG")
        imgs.append(buf.getvalue() if i % 3 else Image.fromarray(arr))
        wms.append(Image.fromarray((_u8(1300 + i, (29, 29)) & 1) * 255, "L"))
    settings = {"block_size": 8, "alpha": 0.15}
    one = pipeline.embed_images(imgs, wms, True, settings, batch_images=None)
    grp = pipeline.embed_images(imgs, wms, True, settings, batch_images=4)
    assert len(one) == len(grp) == 6
    for i, (a, g) in enumerate(zip(one, grp)):
        assert np.array_equal(a.pixels, g.pixels), i
        assert a.png == g.png, i
    assert not np.array_equal(grp[0].pixels, grp[2].pixels)  # one size, two covers and watermarks
    shared = pipeline.embed_images(imgs, wms[0], True, settings, batch_images=4)
    assert np.array_equal(shared[0].pixels, one[0].pixels) and not np.array_equal(shared[1].pixels, one[1].pixels)
