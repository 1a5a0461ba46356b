"""One watermark tile per frame on the GPU: batch.embed_batch / multi.embed_multi with an
(N, H/b, W/b) tile, tmfwm_embed_tiles through ctypes, batch.prepare_tiles.

Frame f with tile f must equal the oracle's single-frame result with that tile.  The covers
(noise / smooth / qr / blocky, camera-like ones for the rank-1 routes) send blocks to the list
pass and to the dgesdd route, whose kernels read the tile too; in every test two frames share
one cover and get different tiles, so an implementation that ignores the stride cannot pass.
"""
import base64
import ctypes

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


def _tiles(n, nbh, nbw, seed):
    """n distinct tiles: uniform bytes and binary 0 / 255 (QR-like) ones alternate."""
    from golden.gen_golden import wmark

    t = np.stack([_u8(seed + i, (nbh, nbw)) if i % 2 == 0 else wmark("qr", nbh, nbw, seed + i) for i in range(n)])
    assert len({x.tobytes() for x in t}) == n
    return t


def _covers(kinds, H, W, seed):
    """Covers by kind; a kind that comes twice gives the same cover twice (frames that differ in their tile only)."""
    from golden.gen_golden import cover
    from lapack_path import photo_cover

    made = {}
    for k in kinds:
        if k not in made:
            made[k] = photo_cover(H, W, seed) if k == "photo" else np.ascontiguousarray(cover(k, H, W, seed + len(made)))
    return np.stack([made[k] for k in kinds])


def _twins(kinds):
    return [(i, j) for i in range(len(kinds)) for j in range(i + 1, len(kinds)) if kinds[i] == kinds[j]]


@pytest.mark.parametrize("b", ALL_B)
def test_every_slider_size_hybrid(dev, b):
    """Frames of 139 x 203 (edge strips on both sides, W/b no multiple of a wave's blocks), a tile
    per frame: embed equals the oracle's frame by frame, and so does extract of the result.  Five
    frames of the kinds noise / smooth / qr / blocky (noise twice: one cover, two tiles), and two
    more for the passes those leave idle at this size: at b = 4 none of the four kinds has a block
    the conditioning test flags (the oracle's hybrid route counts 0), a "diagonal" cover has
    hundreds; a camera-like cover feeds the b = 8 list pass."""
    from thatsmyface_amd import batch

    kinds = ("noise", "smooth", "qr", "blocky", "noise", "diagonal", "photo")
    H, W = 139, 203
    host = _covers(kinds, H, W, 500 + b)
    tiles = _tiles(len(kinds), H // b, W // b, 520 + b)
    fr, tt = torch.from_numpy(host).to(dev), torch.from_numpy(tiles).to(dev)
    st = {}
    out = batch.embed_batch(fr, tt, b, 0.1, stats=st)
    print("stats", b, st)
    assert st["lapack_blocks"] > 0, st
    if b == 8:
        assert st["list_pass_blocks"] > 0, st
    ext = batch.extract_batch(out, fr, b, 0.1).cpu().numpy()
    got = out.cpu().numpy()
    for f in range(len(kinds)):
        ref = O.embed_frame(host[f], tiles[f], b, 0.1)
        assert np.array_equal(got[f], ref), (b, f)
        assert np.array_equal(ext[f], O.extract_frame(ref, host[f], b, 0.1)), (b, f)
    for i, j in _twins(kinds):
        assert not np.array_equal(got[i], got[j]), (b, i, j)


@pytest.mark.parametrize("b", ALL_B)
def test_every_route(dev, b):
    """The reference route with a tile per frame against the oracle's dgesdd route (every slider
    size: each block goes through the fixup kernel's read of the tile); at b = 8 and 16 the hybrid
    and the rank-1 routes against the reference route's bytes, at b = 12 the rank-1 route (its
    list pass lives in another translation unit there)."""
    from thatsmyface_amd import batch

    kinds = ("noise", "smooth", "photo", "blocky", "qr", "photo")
    H, W = 139, 203
    host = _covers(kinds, H, W, 600 + b)
    tiles = _tiles(len(kinds), H // b, W // b, 620 + b)
    fr, tt = torch.from_numpy(host).to(dev), torch.from_numpy(tiles).to(dev)
    st = {}
    ref = batch.embed_batch(fr, tt, b, 0.1, route="reference", stats=st)
    assert st["lapack_blocks"] == len(kinds) * (H // b) * (W // b), st
    got = ref.cpu().numpy()
    for f in range(len(kinds)):
        assert np.array_equal(got[f], O.embed_frame(host[f], tiles[f], b, 0.1, route="lapack")), (b, f)
    for i, j in _twins(kinds):
        assert not np.array_equal(got[i], got[j]), (b, i, j)
    for route in {8: ("hybrid", "rank1", "rank1_reference"), 16: ("hybrid", "rank1", "rank1_reference"), 12: ("rank1",)}.get(b, ()):
        st = {}
        out = batch.embed_batch(fr, tt, b, 0.1, route=route, stats=st)
        print("stats", b, route, st)
        assert st["lapack_blocks"] > 0, (route, st)
        if b == 8 and route != "rank1_reference":
            assert st["list_pass_blocks"] > 0, (route, st)
        assert torch.equal(out, ref), (b, route, st)
    if b == 8:  # the blend's edges: a large alpha, and a negative one that pushes S'[0] below zero
        for alpha in (1.0, -5.0):
            ref_a = batch.embed_batch(fr, tt, b, alpha, route="reference")
            assert torch.equal(batch.embed_batch(fr, tt, b, alpha, route="hybrid"), ref_a), alpha
            f = 2
            assert np.array_equal(ref_a[f].cpu().numpy(), O.embed_frame(host[f], tiles[f], b, alpha, route="lapack")), alpha


def test_chunks(dev, monkeypatch):
    """With TMFWM_DEBUG_LIST_CAP at 1.5 frames' worth of block ids every chunk holds one frame: each
    chunk's passes must read its own frame's tile (the ids in the lists are relative to the chunk)."""
    from thatsmyface_amd import batch

    b, H, W = 8, 272, 480
    kinds = ("smooth", "qr", "smooth", "blocky")
    nb = (H // b) * (W // b)
    host = _covers(kinds, H, W, 30)
    tiles = _tiles(len(kinds), H // b, W // b, 50)
    fr, tt = torch.from_numpy(host).to(dev), torch.from_numpy(tiles).to(dev)
    st0 = {}
    out0 = batch.embed_batch(fr, tt, b, 0.1, stats=st0)
    monkeypatch.setenv("TMFWM_DEBUG_LIST_CAP", str(nb * 3 // 2))
    st1 = {}
    out1 = batch.embed_batch(fr, tt, b, 0.1, stats=st1)
    print("stats", st0, st1)
    assert st0["lapack_blocks"] > 0 and st0["list_pass_blocks"] > 0 and st0 == st1, (st0, st1)
    assert torch.equal(out0, out1)
    got = out1.cpu().numpy()
    for f in range(len(kinds)):
        assert np.array_equal(got[f], O.embed_frame(host[f], tiles[f], b, 0.1)), f
    for i, j in _twins(kinds):
        assert not np.array_equal(got[i], got[j]), (i, j)
    # the rank-1 route's pre-pass and list pass under the same chunking
    r0 = batch.embed_batch(fr, tt, b, 0.1, route="reference")
    assert torch.equal(batch.embed_batch(fr, tt, b, 0.1, route="rank1"), r0)


def test_strides_and_layouts_ctypes(dev):
    """tmfwm_embed_tiles through ctypes: padded tiles in host memory, 4 -> 4 and 3 -> 4 pixel
    layouts; stride 0 is tmfwm_embed_px byte for byte; a tile expanded to (n, nbh, nbw) is the
    shared tile."""
    from thatsmyface_amd import _lib, batch

    L = _lib.load()
    b, H, W = 8, 37, 61
    kinds = ("smooth", "noise", "smooth")
    n, nbh, nbw = len(kinds), H // b, W // b
    tb = nbh * nbw
    rgb = _covers(kinds, H, W, 700)
    tiles = _tiles(n, nbh, nbw, 710)
    refs = np.stack([O.embed_frame(rgb[f], tiles[f], b, 0.1) for f in range(n)])
    assert not np.array_equal(refs[0], refs[2])
    padded = np.full((n, tb + 7), 0xA5, np.uint8)
    padded[:, :tb] = tiles.reshape(n, tb)
    f4, f3 = H * W * 4 + 48, H * W * 3 + 20
    rgbx = np.full((n, f4), 77, np.uint8)
    rgbx[:, : H * W * 4].reshape(n, H * W, 4)[..., :3] = rgb.reshape(n, H * W, 3)
    rgb3 = np.zeros((n, f3), np.uint8)
    rgb3[:, : H * W * 3] = rgb.reshape(n, -1)
    ostride = H * W * 4 + 16
    for src, ipx, sstride in ((rgbx, 4, f4), (rgb3, 3, f3)):
        for mem in ("host", "device"):
            out = np.zeros((n, ostride), np.uint8)
            cnt = ctypes.c_int64(0)
            if mem == "host":
                _lib.check(L.tmfwm_embed_tiles(src.ctypes.data, ipx, sstride, n, H, W, padded.ctypes.data, tb + 7, b, 0.1,
                                               out.ctypes.data, 4, ostride, _lib.MEM_HOST, None, 0, ctypes.addressof(cnt)), "embed_tiles")
            else:
                ds, dt, do = (torch.from_numpy(x).to(dev) for x in (src, padded, out))
                _lib.check(L.tmfwm_embed_tiles(ds.data_ptr(), ipx, sstride, n, H, W, dt.data_ptr(), tb + 7, b, 0.1, do.data_ptr(), 4,
                                               ostride, _lib.MEM_DEVICE, None, 0, ctypes.addressof(cnt)), "embed_tiles")
                torch.cuda.synchronize()
                out = do.cpu().numpy()
            px = out[:, : H * W * 4].reshape(n, H, W, 4)
            assert cnt.value > 0, (ipx, mem)
            assert np.array_equal(px[..., :3], refs), (ipx, mem)
            assert (px[..., 3] == 255).all() and (out[:, H * W * 4:] == 0).all(), (ipx, mem)
    # 3 -> 3 with padded tiles on the device (embed_batch passes compact ones)
    d3, dt, do = (torch.from_numpy(x).to(dev) for x in (rgb3, padded, np.zeros_like(rgb3)))
    _lib.check(L.tmfwm_embed_tiles(d3.data_ptr(), 3, f3, n, H, W, dt.data_ptr(), tb + 7, b, 0.1, do.data_ptr(), 3, f3, _lib.MEM_DEVICE,
                                   None, 0, None), "embed_tiles")
    torch.cuda.synchronize()
    o3 = do.cpu().numpy()
    assert np.array_equal(o3[:, : H * W * 3].reshape(n, H, W, 3), refs) and (o3[:, H * W * 3:] == 0).all()
    # the output may not overlap any frame's tile: here it starts inside the last one, clear of the first two
    big = torch.zeros(2 * (tb + 7) + 1 + n * f3, dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match="overlaps"):
        _lib.check(L.tmfwm_embed_tiles(d3.data_ptr(), 3, f3, n, H, W, big.data_ptr(), tb + 7, b, 0.1,
                                       big.data_ptr() + 2 * (tb + 7) + 1, 3, f3, _lib.MEM_DEVICE, None, 0, None), "embed_tiles")
    # stride 0: one shared tile, exactly tmfwm_embed_px
    a, c = np.zeros((n, ostride), np.uint8), np.zeros((n, ostride), np.uint8)
    _lib.check(L.tmfwm_embed_tiles(rgbx.ctypes.data, 4, f4, n, H, W, padded.ctypes.data, 0, b, 0.1, a.ctypes.data, 4, ostride,
                                   _lib.MEM_HOST, None, 0, None), "embed_tiles")
    _lib.check(L.tmfwm_embed_px(rgbx.ctypes.data, 4, f4, n, H, W, padded.ctypes.data, b, 0.1, c.ctypes.data, 4, ostride, _lib.MEM_HOST,
                                None, 0, None), "embed_px")
    assert np.array_equal(a, c)
    assert np.array_equal(a[1, : H * W * 4].reshape(H, W, 4)[..., :3], O.embed_frame(rgb[1], tiles[0], b, 0.1))
    fr, t0 = torch.from_numpy(rgb).to(dev), torch.from_numpy(tiles[0]).to(dev)
    assert torch.equal(batch.embed_batch(fr, t0.expand(n, -1, -1).contiguous(), b, 0.1), batch.embed_batch(fr, t0, b, 0.1))
    for bad in (tiles[:2], tiles[:, :-1], tiles[None]):
        with pytest.raises(ValueError, match="wm_tile"):
            batch.embed_batch(fr, torch.from_numpy(np.ascontiguousarray(bad)).to(dev), b, 0.1)


@pytest.mark.parametrize("ih,iw,oh,ow", [(29, 29, 17, 25), (300, 300, 17, 25), (300, 300, 135, 240), (17, 25, 17, 25)])
def test_prepare_tiles(dev, ih, iw, oh, ow):
    """Three watermarks per launch: every tile is the oracle's Pillow restatement of its own
    watermark and batch.prepare_tile's (upscale of one axis with paste offsets, downscale, copy)."""
    from thatsmyface_amd import batch

    wms = np.stack([_u8(800 + ih + i, (ih, iw)) if i != 1 else (_u8(810 + ih, (ih, iw)) & 1) * 255 for i in range(3)]).astype(np.uint8)
    dw = torch.from_numpy(wms).to(dev)
    for pr in (False, True):
        got = batch.prepare_tiles(dw, oh, ow, pr)
        assert got.shape == (3, oh, ow)
        for i in range(3):
            assert np.array_equal(got[i].cpu().numpy(), O.prepare_tile(wms[i], oh, ow, pr)), (i, pr)
            assert torch.equal(got[i], batch.prepare_tile(dw[i], oh, ow, pr)), (i, pr)
        out = torch.full((3, oh, ow), 7, dtype=torch.uint8, device=dev)
        assert batch.prepare_tiles(dw, oh, ow, pr, out=out) is out and torch.equal(out, got)
    for shape in ((2, oh, ow), (3, ow, oh + 1), (3, oh * ow)):
        with pytest.raises(ValueError, match="out"):
            batch.prepare_tiles(dw, oh, ow, True, out=torch.empty(shape, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError):
        batch.prepare_tiles(dw[0], oh, ow)


def test_prepare_tiles_padded_strides(dev):
    """tmfwm_prepare_tiles with padded watermark and tile strides, host and device memory: the
    bytes between the tiles are not written."""
    from thatsmyface_amd import _lib

    L = _lib.load()
    n, ih, iw, oh, ow = 3, 29, 31, 17, 25
    ws, ts = ih * iw + 5, oh * ow + 9
    wm = np.full((n, ws), 3, np.uint8)
    wm[:, : ih * iw] = _u8(830, (n, ih * iw))
    for pr in (0, 1):
        ref = np.stack([O.prepare_tile(wm[i, : ih * iw].reshape(ih, iw), oh, ow, bool(pr)) for i in range(n)]).reshape(n, -1)
        out = np.full((n, ts), 0x5A, np.uint8)
        _lib.check(L.tmfwm_prepare_tiles(wm.ctypes.data, n, ih, iw, ws, oh, ow, pr, out.ctypes.data, ts, _lib.MEM_HOST, None), "prepare_tiles")
        assert np.array_equal(out[:, : oh * ow], ref) and (out[:, oh * ow:] == 0x5A).all(), pr
        dwm, dout = torch.from_numpy(wm).to(dev), torch.full((n, ts), 0x5A, dtype=torch.uint8, device=dev)
        _lib.check(L.tmfwm_prepare_tiles(dwm.data_ptr(), n, ih, iw, ws, oh, ow, pr, dout.data_ptr(), ts, _lib.MEM_DEVICE, None),
                   "prepare_tiles")
        assert np.array_equal(dout.cpu().numpy(), out), pr


def test_multi_entry_point(dev, monkeypatch):
    """multi.embed_multi with a tile per frame: logical shards on device 0 and passes of two frames
    (both slots, a short last pass) equal the device-resident batch call and the oracle; no
    broadcast runs in this mode, and a 2-D tile still takes the broadcast path."""
    from thatsmyface_amd import batch, multi

    b, H, W = 8, 136, 200
    kinds = ("noise", "smooth", "qr", "noise", "smooth", "blocky", "noise")
    n = len(kinds)
    host = _covers(kinds, H, W, 40)
    tiles = _tiles(n, H // b, W // b, 60)
    sd = {}
    ref_dev = batch.embed_batch(torch.from_numpy(host).to(dev), torch.from_numpy(tiles).to(dev), b, 0.1, stats=sd).cpu().numpy()
    assert sd["lapack_blocks"] > 0, sd
    for f in range(n):
        assert np.array_equal(ref_dev[f], O.embed_frame(host[f], tiles[f], b, 0.1)), f
    for i, j in _twins(kinds):
        assert not np.array_equal(ref_dev[i], ref_dev[j]), (i, j)
    one = H * W * 3
    monkeypatch.setenv("TMFWM_DEBUG_FORCE_RCCL", "0")
    for shards, pass_bytes in (([0, 0, 0], ""), ([0], ""), ([0, 0], str(4 * one))):
        monkeypatch.setenv("TMFWM_DEBUG_PASS_BYTES", pass_bytes)
        st = {}
        out = multi.embed_multi(host, tiles, b, 0.1, devices=shards, stats=st)
        assert np.array_equal(out, ref_dev), shards
        assert st["lapack_blocks"] == sd["lapack_blocks"], (shards, st, sd)
    assert np.array_equal(multi.embed_multi(host, tiles, b, 0.1, devices=[0, 0], route="rank1"),
                          multi.embed_multi(host, tiles, b, 0.1, devices=[0], route="reference"))
    assert torch.cuda.current_device() == 0
    # one shared tile: the broadcast path (RCCL even on one device when forced), unchanged
    monkeypatch.setenv("TMFWM_DEBUG_FORCE_RCCL", "1")
    shared = batch.embed_batch(torch.from_numpy(host).to(dev), torch.from_numpy(tiles[1]).to(dev), b, 0.1).cpu().numpy()
    assert np.array_equal(multi.embed_multi(host, tiles[1], b, 0.1, devices=[0, 0]), shared)


# four fixed payloads: an AES-CBC ciphertext under a fixed IV each (encrypt_watermark draws a random one)
_KEY = bytes(range(7, 39))
_TEXTS = ("user 0001 / session a", "user 0002 / session b", "user 0003 / session c", "user 0004 / session d")


def _payloads():
    from thatsmyface_amd import encryption as E

    out = []
    for i, text in enumerate(_TEXTS):
        iv = bytes((17 * i + k) & 255 for k in range(16))
        out.append(iv + E.aes_cbc_encrypt(_KEY, iv, E.pad(text.encode())))
    return out


def test_end_to_end_payload_per_frame(dev):
    """Four users' payloads in one batch: text_to_qrcode -> prepare_tiles -> embed_batch with a tile
    per frame -> extract_batch -> decode_tiles; frame i gives payload i back."""
    from lapack_path import photo_cover

    from thatsmyface_amd import batch
    from thatsmyface_amd import encryption as E
    from thatsmyface_amd import qrcode_generator as Q

    enc = _payloads()
    assert len(set(enc)) == 4
    wms = np.stack([np.asarray(Q.text_to_qrcode(e).convert("L"), dtype=np.uint8) for e in enc])
    assert wms.shape == (4, 300, 300)
    frames = torch.from_numpy(np.stack([photo_cover(1080, 1920, s) for s in range(4)])).to(dev)
    tiles = batch.prepare_tiles(torch.from_numpy(wms).to(dev), 1080 // 8, 1920 // 8, True)
    assert len({t.cpu().numpy().tobytes() for t in tiles}) == 4
    ext = batch.extract_batch(batch.embed_batch(frames, tiles, 8, 0.1), frames, 8, 0.1)
    assert Q.decode_tiles(ext.cpu().numpy()) == [base64.b64encode(e) for e in enc]
    for i, e in enumerate(enc):
        assert E.decrypt_watermark(e, _KEY) == _TEXTS[i].encode()
