"""Embed that also returns the extraction key, on the GPU: batch.embed_with_key /
embed_with_key_ragged, tmfwm_embed_key / tmfwm_embed_key_ragged through ctypes, the drop-in's
embed_watermark_with_key and pipeline.embed_images(..., return_keys=True).

Expected values exist already: the bytes are batch.embed_batch's / embed_ragged's, the key bits
keyed_helpers.key_of's (the oracle's dgesdd route) and batch.sigma1_map's."""
import ctypes
import io
import os
import sys

import numpy as np
import pytest
from PIL import Image

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import embed_key_helpers as EK  # noqa: E402
from keyed_helpers import key_of, sparks  # noqa: E402
from test_keyed_gpu import _shapes, _three_covers  # noqa: E402
from test_ragged_gpu import _desc, _dev, _frames, _mixed_specs  # noqa: E402

BLOCKS = (4, 6, 8, 10, 12, 14, 16)
ROUTES = ("hybrid", "reference", "rank1", "rank1_reference")
ALPHAS = (0.1, 1.0, -0.5)


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


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.mark.parametrize("b", BLOCKS)
def test_every_route_shape_alpha_and_tile_form(dev, b):
    """Three covers (noise, camera-like, QR) with per-frame tiles and with one shared tile, every
    route name, alpha 0.1 / 1.0 / -0.5, both shapes: out is embed_batch's bytes, the key is key_of's
    and sigma1_map's bits -- whatever the route, the alpha and the tile."""
    from golden.gen_golden import wmark

    from thatsmyface_amd import batch

    for H, W in _shapes(b):
        nbh, nbw = H // b, W // b
        host = _three_covers(H, W, 30 * b)
        fr = torch.from_numpy(host).to(dev)
        ref = np.stack([key_of(host[f], b) for f in range(3)])
        smap = batch.sigma1_map(fr, b)
        assert np.array_equal(_bits(smap), _bits(ref)), (H, W)
        tiles = torch.from_numpy(np.stack([wmark(k, nbh, nbw, 5 + i) for i, k in enumerate(("noise", "qr", "pattern"))])).to(dev)
        for tt in (tiles, tiles[1].contiguous()):
            for alpha in ALPHAS:
                for route in ROUTES:
                    se, sk = {}, {}
                    exp = batch.embed_batch(fr, tt, b, alpha, route=route, stats=se)
                    out, key = batch.embed_with_key(fr, tt, b, alpha, route=route, stats=sk)
                    where = (H, W, tt.dim(), alpha, route)
                    assert key.dtype == torch.float32 and tuple(key.shape) == (3, nbh, nbw)
                    assert torch.equal(out, exp), where
                    assert np.array_equal(_bits(key), _bits(ref)), where
                    if route == "reference":
                        assert sk["lapack_blocks"] == 3 * nbh * nbw and sk["list_pass_blocks"] == 0, (where, sk)
                    elif route == "hybrid":  # the fused route: only key-undecided blocks are added to embed's
                        assert se["lapack_blocks"] <= sk["lapack_blocks"] <= se["lapack_blocks"] + 2, (where, se, sk)
                        assert sk["list_pass_blocks"] == se["list_pass_blocks"], (where, se, sk)
                    else:  # composed: embed's passes, then the map's
                        assert sk["lapack_blocks"] >= se["lapack_blocks"], (where, se, sk)
        # asynchronous (no count), into the caller's buffers
        out = torch.full_like(fr, 7)
        kbuf = torch.full((3, nbh, nbw), -7.0, dtype=torch.float32, device=dev)
        o2, k2 = batch.embed_with_key(fr, tiles, b, 0.1, out=out, key_out=kbuf)
        assert o2 is out and k2 is kbuf
        torch.cuda.synchronize()
        assert torch.equal(out, batch.embed_batch(fr, tiles, b, 0.1)) and np.array_equal(_bits(kbuf), _bits(ref))


@pytest.mark.parametrize("b", BLOCKS)
def test_special_blocks(dev, b):
    """The tE = 0 paths: a black frame (zero blocks), a flat-colour frame (flat blocks) and a flat
    frame with one changed pixel per block."""
    from thatsmyface_amd import batch

    H, W = _shapes(b)[0]
    nbh, nbw = H // b, W // b
    black = np.zeros((H, W, 3), np.uint8)
    flat = np.empty((H, W, 3), np.uint8)
    flat[...] = (37, 201, 90)
    dot = flat.copy()
    rng = np.random.default_rng(b)
    for bi in range(nbh):
        for bj in range(nbw):
            dot[bi * b + rng.integers(b), bj * b + rng.integers(b)] = rng.integers(0, 256, 3)
    host = np.ascontiguousarray(np.stack([black, flat, dot]))
    cert = np.stack([EK.predict(host[f], b)[0] for f in range(3)])
    assert not cert[0].any() and not cert[1].any()  # zero and flat blocks: point intervals
    fr = torch.from_numpy(host).to(dev)
    tile = torch.from_numpy(_u8(9, (nbh, nbw))).to(dev)
    ref = np.stack([key_of(host[f], b) for f in range(3)])
    assert (ref[0] == 0).all()
    for route in ROUTES:
        for alpha in (0.1, -0.5):
            out, key = batch.embed_with_key(fr, tile, b, alpha, route=route)
            assert np.array_equal(_bits(key), _bits(ref)), (route, alpha)
            assert torch.equal(out, batch.embed_batch(fr, tile, b, alpha, route=route)), (route, alpha)


@pytest.mark.parametrize("b", BLOCKS)
def test_sparks_frame_every_block_flagged(dev, b):
    """All singular values of a sparks block are equal: every block is flagged, so the dgesdd
    route's pass writes the whole key, over what the strip pass stored."""
    from thatsmyface_amd import batch

    H, W = _shapes(b)[0]
    nbh, nbw = H // b, W // b
    host = np.ascontiguousarray(np.stack([sparks(H, W, b, 60 + f) for f in range(2)]))
    fr = torch.from_numpy(host).to(dev)
    tile = torch.from_numpy(_u8(10, (nbh, nbw))).to(dev)
    st, se = {}, {}
    out, key = batch.embed_with_key(fr, tile, b, 0.1, stats=st)
    assert torch.equal(out, batch.embed_batch(fr, tile, b, 0.1, stats=se))
    assert st["lapack_blocks"] == 2 * nbh * nbw == se["lapack_blocks"], (st, se)
    for f in range(2):
        assert np.array_equal(_bits(key[f]), _bits(key_of(host[f], b))), f


@pytest.mark.parametrize("b", (8,))  # (b = 16: the search found 2 hits in 9.4 M blocks and 12 minutes; no fixture)
def test_undecided_key_goes_to_the_dgesdd_route(dev, b):
    """tests/golden/embed_key_undecided_b<b>.npz (tools/exp/embed_key_undecided.py): noise blocks
    whose sigma_1 lies within 2^-45 sigma_1 of a float midpoint, found by a seeded CPU search and
    tiled among ordinary noise blocks.  The strip pass certifies their bytes but cannot decide
    their key: they must join the dgesdd-route list, whose pass stores np.linalg.svd's own S[0].
    (Storing the lower end instead fails here on bits wherever LAPACK's sigma_1 rounds up.)"""
    from thatsmyface_amd import batch

    fx = np.load(os.path.join(ROOT, "tests", "golden", f"embed_key_undecided_b{b}.npz"))
    frame, und = np.ascontiguousarray(fx["frame"]), fx["undecided"]
    assert int(fx["block"]) == b and len(und) >= 4 and int(fx["hits"]) >= 4 and int(fx["blocks_searched"]) > 0
    cert, dec, pkey = EK.predict(frame, b)
    assert sorted(map(tuple, np.argwhere(cert & ~dec))) == sorted(map(tuple, und))  # the helper still predicts them
    H, W = frame.shape[:2]
    ref = key_of(frame, b)
    # the two ends of such a block are neighbouring floats and LAPACK's S[0] is one of them
    lo = pkey[tuple(und.T)]
    assert all(r in (l, np.nextafter(l, np.float32(np.inf))) for r, l in zip(ref[tuple(und.T)], lo))
    fr = torch.from_numpy(frame[None].copy()).to(dev)
    tile = torch.from_numpy(_u8(11, (H // b, W // b))).to(dev)
    for alpha in (0.1, -0.5):
        st, se = {}, {}
        out, key = batch.embed_with_key(fr, tile, b, alpha, stats=st)
        exp = batch.embed_batch(fr, tile, b, alpha, stats=se)
        print("undecided", b, alpha, st, se, "lower end is the key at", int((ref[tuple(und.T)] == lo).sum()), "of", len(und))
        assert np.array_equal(_bits(key[0]), _bits(ref)), alpha
        assert torch.equal(out, exp), alpha
        assert st["lapack_blocks"] >= len(und), (st, len(und))
        assert st["lapack_blocks"] > se["lapack_blocks"], (st, se)
    for route in ROUTES[1:]:
        assert np.array_equal(_bits(batch.embed_with_key(fr, tile, b, 0.1, route=route)[1][0]), _bits(ref)), route


def test_b8_list_pass_hands_the_key_over(dev):
    """b = 8 on test_gpu_parity's smallest list-pass shape: the strip pass defers blocks
    (camera-like covers need a second sweep) and writes nothing for them; their key entries come
    from the list pass."""
    from golden.gen_golden import wmark
    from lapack_path import photo_cover

    from thatsmyface_amd import batch

    b, H, W = 8, 544, 960
    host = np.ascontiguousarray(np.stack([_u8(71, (H, W, 3)), photo_cover(H, W, 5)]))
    fr = torch.from_numpy(host).to(dev)
    tile = torch.from_numpy(wmark("qr", H // b, W // b, 9)).to(dev)
    st, se = {}, {}
    key = torch.full((2, H // b, W // b), float("nan"), dtype=torch.float32, device=dev)
    out, _ = batch.embed_with_key(fr, tile, b, 0.1, key_out=key, stats=st)
    assert st["list_pass_blocks"] > 0, st
    assert torch.equal(out, batch.embed_batch(fr, tile, b, 0.1, stats=se))
    assert st["list_pass_blocks"] == se["list_pass_blocks"], (st, se)
    assert _same_bits(key, batch.sigma1_map(fr, b))
    for f in range(2):
        assert np.array_equal(_bits(key[f]), _bits(key_of(host[f], b))), f


def test_chunked_calls_and_padded_key_stride(dev, monkeypatch):
    """TMFWM_DEBUG_LIST_CAP at 1.5 frames' worth of ids (test_keyed_gpu's knob): one frame per
    chunk; each chunk's key offset must be its own -- on the fused routes and on the composed
    one -- and a padded key_stride keeps its padding."""
    from golden.gen_golden import cover

    from thatsmyface_amd import _lib, batch

    b, H, W = 8, 64, 128
    nbh, nbw = H // b, W // b
    nb = nbh * nbw
    host = np.ascontiguousarray(np.stack([cover("smooth", H, W, 30), sparks(H, W, b, 31), cover("qr", H, W, 32), _u8(33, (H, W, 3))]))
    fr = torch.from_numpy(host).to(dev)
    tiles = torch.from_numpy(_u8(34, (4, nbh, nbw))).to(dev)
    ref = np.stack([key_of(host[f], b) for f in range(4)])

    def run(route):
        st = {}
        out, key = batch.embed_with_key(fr, tiles, b, 0.1, stats=st, route=route)
        return out, key, st

    whole = {r: run(r) for r in ROUTES}
    monkeypatch.setenv("TMFWM_DEBUG_LIST_CAP", str(nb * 3 // 2))
    L = _lib.load()
    pad = 5
    for route in ROUTES:
        out, key, st = run(route)
        assert st == whole[route][2] and st["lapack_blocks"] >= nb, (route, st, whole[route][2])
        assert torch.equal(out, whole[route][0]) and torch.equal(out, batch.embed_batch(fr, tiles, b, 0.1, route=route)), route
        assert np.array_equal(_bits(key), _bits(ref)), route
        # a padded stride through the C ABI: device memory, then host memory
        padded = torch.full((4, nb + pad), -7.0, dtype=torch.float32, device=dev)
        o2 = torch.empty_like(fr)
        cnt = ctypes.c_int64(-1)
        with torch.cuda.device(dev):
            _lib.check(L.tmfwm_embed_key(fr.data_ptr(), 4, H, W, H * W * 3, tiles.data_ptr(), nb, b, 0.1, o2.data_ptr(),
                                         padded.data_ptr(), (nb + pad) * 4, _lib.MEM_DEVICE, None, _lib.route_code(route),
                                         ctypes.addressof(cnt)), "embed_key")
        assert cnt.value == st["lapack_blocks"] and torch.equal(o2, out), route
        assert np.array_equal(_bits(padded[:, :nb]), _bits(ref.reshape(4, nb))) and (padded[:, nb:] == -7.0).all(), route
        hp = np.full((4, nb + pad), -7.0, np.float32)
        ho = np.zeros_like(host)
        ht = tiles.cpu().numpy()
        cnt = ctypes.c_int64(-1)
        _lib.check(L.tmfwm_embed_key(host.ctypes.data, 4, H, W, H * W * 3, ht.ctypes.data, nb, b, 0.1, ho.ctypes.data, hp.ctypes.data,
                                     (nb + pad) * 4, _lib.MEM_HOST, None, _lib.route_code(route), ctypes.addressof(cnt)), "embed_key")
        assert cnt.value == st["lapack_blocks"] and np.array_equal(ho, out.cpu().numpy()), route
        assert np.array_equal(_bits(hp[:, :nb]), _bits(ref.reshape(4, nb))) and (hp[:, nb:] == -7.0).all(), route


@pytest.mark.parametrize("b", BLOCKS)
def test_ragged_mixed_shapes(dev, b):
    """test_ragged_gpu's mixed frame list (among it a frame smaller than a block, a one-block
    frame and W % 4 != 0): per-frame bytes are embed_ragged's, keys sigma1_map_ragged's and key_of's."""
    from thatsmyface_amd import _lib, batch

    specs = _mixed_specs(b)
    covers, tiles = _frames(specs, b, 900 + b)
    fr, tt = _dev(covers, dev), _dev(tiles, dev)
    nob = next(i for i, (_, H, W, _) in enumerate(specs) if H < b)
    nblocks = sum((H // b) * (W // b) for _, H, W, _ in specs)
    se, st, sr = {}, {}, {}
    exp = batch.embed_ragged(fr, tt, b, 0.1, stats=se)
    smap = batch.sigma1_map_ragged(fr, b)
    outs, keys = batch.embed_with_key_ragged(fr, tt, b, 0.1, stats=st)
    assert st["list_pass_blocks"] == 0 and se["lapack_blocks"] <= st["lapack_blocks"] <= se["lapack_blocks"] + 2, (se, st)
    ro, rk = batch.embed_with_key_ragged(fr, tt, b, 0.1, stats=sr, route="reference")
    assert sr == {"lapack_blocks": nblocks, "list_pass_blocks": 0}, sr
    rexp = batch.embed_ragged(fr, tt, b, 0.1, route="reference")
    for i, (kind, H, W, _) in enumerate(specs):
        assert keys[i].dtype == torch.float32 and tuple(keys[i].shape) == (H // b, W // b) and keys[i].data_ptr() % 4 == 0
        assert torch.equal(outs[i], exp[i]) and torch.equal(ro[i], rexp[i]), (b, i)
        assert _same_bits(keys[i], smap[i]) and _same_bits(rk[i], smap[i]), (b, i)
        if H >= b and W >= b:
            assert np.array_equal(_bits(keys[i]), _bits(key_of(covers[i], b))), (b, i)
    assert keys[nob].numel() == 0
    # asynchronous, into caller buffers through the C ABI; sentinels past each key and in the
    # buffer of the frame without a block stay untouched
    obuf = [torch.full_like(f, 3) for f in fr]
    kbuf = [torch.full((max(k.numel(), 6) + 2,), -7.0, dtype=torch.float32, device=dev) for k in keys]
    rows = [(f.data_ptr(), o.data_ptr(), t.data_ptr() if t.numel() else None, k.data_ptr(), f.shape[0], f.shape[1])
            for f, o, t, k in zip(fr, obuf, tt, kbuf)]
    d = _desc(_lib.EmbedKeyFrame, rows)
    L = _lib.load()
    with torch.cuda.device(dev):
        _lib.check(L.tmfwm_embed_key_ragged(ctypes.addressof(d), len(rows), b, 0.1, _lib.MEM_DEVICE,
                                            torch.cuda.current_stream().cuda_stream, _lib.ROUTE_HYBRID, None), "embed_key_ragged")
    torch.cuda.synchronize()
    for i in range(len(specs)):
        n = keys[i].numel()
        assert torch.equal(obuf[i], exp[i]), (b, i)
        assert _same_bits(kbuf[i][:n].view(keys[i].shape), keys[i]) and (kbuf[i][n:] == -7.0).all(), (b, i)
    assert (kbuf[nob] == -7.0).all()
    # through batch with out= / key_out=
    o3, k3 = batch.embed_with_key_ragged(fr, tt, b, 0.1, out=obuf, key_out=[k[:keys[i].numel()].view(keys[i].shape) for i, k in enumerate(kbuf)])
    assert all(a is o for a, o in zip(o3, obuf)) and all(_same_bits(a, k) for a, k in zip(k3, keys))


def test_ragged_position_independence(dev):
    from thatsmyface_amd import batch

    for b in (8, 14):
        specs = _mixed_specs(b)
        covers, tiles = _frames(specs, b, 940 + b)
        fr, tt = _dev(covers, dev), _dev(tiles, dev)
        bo, bk = batch.embed_with_key_ragged(fr, tt, b, 0.1)
        n = len(specs)
        for order in (list(range(n))[::-1], [int(k) for k in np.random.default_rng(5).permutation(n)]):
            outs, keys = batch.embed_with_key_ragged([fr[k] for k in order], [tt[k] for k in order], b, 0.1)
            for pos, k in enumerate(order):
                assert torch.equal(outs[pos], bo[k]) and _same_bits(keys[pos], bk[k]), (b, order, pos)


def test_host_memory_overlaps_and_pointer_kinds(dev):
    from thatsmyface_amd import _lib, batch

    L = _lib.load()
    b, H, W, n = 8, 24, 40, 2
    nbh, nbw = H // b, W // b
    kb = nbh * nbw * 4
    host = _u8(70, (n, H, W, 3))
    buf = torch.zeros(n * H * W * 3 + 64, dtype=torch.uint8, device=dev)
    fr = buf[: n * H * W * 3].view(n, H, W, 3)
    fr.copy_(torch.from_numpy(host))
    tile = torch.from_numpy(_u8(71, (nbh, nbw))).to(dev)
    exp, ref = batch.embed_batch(fr, tile, b, 0.1), batch.sigma1_map(fr, b)
    out = torch.empty_like(fr)
    # key over the input, key over out, out over the input: refused
    with pytest.raises(ValueError, match="overlaps"):
        batch.embed_with_key(fr, tile, b, 0.1, out=out, key_out=buf[16: 16 + n * kb].view(torch.float32).view(n, nbh, nbw))
    with pytest.raises(ValueError, match="overlaps"):
        batch.embed_with_key(fr, tile, b, 0.1, out=out, key_out=out.view(-1)[32: 32 + n * kb].view(torch.float32).view(n, nbh, nbw))
    with pytest.raises(ValueError, match="overlaps"):
        batch.embed_with_key(fr, tile, b, 0.1, out=fr)
    ktile = torch.zeros((n, nbh, nbw), dtype=torch.float32, device=dev)
    with pytest.raises(ValueError, match="overlaps"):
        batch.embed_with_key(fr, ktile.view(torch.uint8).view(-1)[: nbh * nbw].view(nbh, nbw), b, 0.1, out=out, key_out=ktile)
    # ragged: key over out, key over an input, two frames' keys
    frs, outs = [fr[0], fr[1]], [out[0], out[1]]
    k0, k1 = ktile[0], ktile[1]
    with pytest.raises(ValueError, match="overlaps"):
        batch.embed_with_key_ragged(frs, [tile, tile], b, 0.1, out=outs, key_out=[k0, out[0].view(-1)[: kb].view(torch.float32).view(nbh, nbw)])
    with pytest.raises(ValueError, match="overlaps"):
        batch.embed_with_key_ragged(frs, [tile, tile], b, 0.1, out=outs, key_out=[k0, fr[0].view(-1)[: kb].view(torch.float32).view(nbh, nbw)])
    with pytest.raises(ValueError, match="overlaps"):
        batch.embed_with_key_ragged(frs, [tile, tile], b, 0.1, out=outs, key_out=[k0, k0])
    with pytest.raises(ValueError, match="overlaps"):
        batch.embed_with_key_ragged(frs, [tile, tile], b, 0.1, out=outs,
                                    key_out=[k0, ktile.view(-1)[nbh * nbw - 1: 2 * nbh * nbw - 1].view(nbh, nbw)])
    # a host pointer passed as device memory is refused, not dereferenced
    hk = np.zeros((n, nbh, nbw), np.float32)
    with torch.cuda.device(dev):
        with pytest.raises(ValueError, match="device"):
            _lib.check(L.tmfwm_embed_key(fr.data_ptr(), n, H, W, H * W * 3, tile.data_ptr(), 0, b, 0.1, out.data_ptr(), hk.ctypes.data,
                                         kb, _lib.MEM_DEVICE, None, 0, None), "k")
        with pytest.raises(ValueError, match="device"):
            _lib.check(L.tmfwm_embed_key(host.ctypes.data, n, H, W, H * W * 3, tile.data_ptr(), 0, b, 0.1, out.data_ptr(),
                                         ktile.data_ptr(), kb, _lib.MEM_DEVICE, None, 0, None), "k")
        d = _desc(_lib.EmbedKeyFrame, [(fr[0].data_ptr(), out[0].data_ptr(), tile.data_ptr(), hk.ctypes.data, H, W)])
        with pytest.raises(ValueError, match="device"):
            _lib.check(L.tmfwm_embed_key_ragged(ctypes.addressof(d), 1, b, 0.1, _lib.MEM_DEVICE, None, 0, None), "r")
        # a misaligned device key pointer
        with pytest.raises(ValueError, match="4-byte aligned"):
            _lib.check(L.tmfwm_embed_key(fr.data_ptr(), n, H, W, H * W * 3, tile.data_ptr(), 0, b, 0.1, out.data_ptr(),
                                         ktile.data_ptr() + 2, kb, _lib.MEM_DEVICE, None, 0, None), "k")
    # host memory on both calls, with a count
    ht = tile.cpu().numpy()
    ho = np.zeros_like(host)
    cnt = ctypes.c_int64(-1)
    _lib.check(L.tmfwm_embed_key(host.ctypes.data, n, H, W, H * W * 3, ht.ctypes.data, 0, b, 0.1, ho.ctypes.data, hk.ctypes.data, kb,
                                 _lib.MEM_HOST, None, 0, ctypes.addressof(cnt)), "k")
    assert cnt.value >= 0 and np.array_equal(ho, exp.cpu().numpy()) and np.array_equal(_bits(hk), _bits(ref))
    specs = [("qr", 40, 64, 0), ("diagonal", 139, 203, 0), ("blocky", 37, 61, 0), ("noise", 5, 9, 0)]
    covers, tiles = _frames(specs, b, 1000)
    rexp = batch.embed_ragged(_dev(covers, dev), _dev(tiles, dev), b, 0.1)
    houts = [np.zeros_like(c) for c in covers]
    hkeys = [np.full((max((c.shape[0] // b) * (c.shape[1] // b), 4),), -7.0, np.float32) for c in covers]
    d = _desc(_lib.EmbedKeyFrame, [(c.ctypes.data, o.ctypes.data, t.ctypes.data if t.size else None, k.ctypes.data, c.shape[0], c.shape[1])
                                   for c, o, t, k in zip(covers, houts, tiles, hkeys)])
    cnt = ctypes.c_int64(-1)
    _lib.check(L.tmfwm_embed_key_ragged(ctypes.addressof(d), len(specs), b, 0.1, _lib.MEM_HOST, None, 0, ctypes.addressof(cnt)), "r")
    assert cnt.value > 0
    for i, c in enumerate(covers):
        nb = (c.shape[0] // b) * (c.shape[1] // b)
        assert np.array_equal(houts[i], rexp[i].cpu().numpy()), i
        assert np.array_equal(_bits(hkeys[i][:nb]), _bits(key_of(c, b).reshape(-1))) and (hkeys[i][nb:] == -7.0).all(), i


def test_round_trip_through_the_keyed_extract(dev):
    from thatsmyface_amd import batch

    for b in (4, 8, 14):
        H, W = _shapes(b)[0]
        host = _three_covers(H, W, 50 * b)
        fr = torch.from_numpy(host).to(dev)
        tiles = torch.from_numpy(_u8(12, (3, H // b, W // b))).to(dev)
        out, key = batch.embed_with_key(fr, tiles, b, 0.1)
        assert torch.equal(batch.extract_keyed(out, key, b, 0.1), batch.extract_batch(out, fr, b, 0.1)), b
        specs = _mixed_specs(b)
        covers, tl = _frames(specs, b, 960 + b)
        rf, rt = _dev(covers, dev), _dev(tl, dev)
        outs, keys = batch.embed_with_key_ragged(rf, rt, b, 0.1)
        got, pair = batch.extract_keyed_ragged(outs, keys, b, 0.1), batch.extract_ragged(outs, rf, b, 0.1)
        assert all(torch.equal(g, p) for g, p in zip(got, pair)), b


def test_dropin_on_golden(dev, golden_alpha):
    """embed_watermark_with_key == (embed_watermark, extraction_key) on one golden fixture per
    block size, on both routes of the drop-in."""
    from thatsmyface_amd import watermarking as W

    cases, meta = golden_alpha
    seen = set()
    for name, m in meta["cases"].items():
        if m["block"] in seen:
            continue
        seen.add(m["block"])
        arr = cases[f"{name}/cover"]
        cov = Image.fromarray(arr, "L" if arr.ndim == 2 else ("RGBA" if arr.shape[-1] == 4 else "RGB"))
        wm = Image.fromarray(cases[f"{name}/wm"])
        for route in ("reference", "hybrid"):
            s = {"block_size": m["block"], "alpha": m["alpha"], "svd_route": route}
            img, key = W.embed_watermark_with_key(cov, wm, m["preserve_ratio"], s)
            exp = W.embed_watermark(cov, wm, m["preserve_ratio"], s)
            assert img.mode == "RGB" and img.size == exp.size
            assert np.array_equal(np.asarray(img), np.asarray(exp)), (name, route)
            assert key.dtype == np.float32 and np.array_equal(_bits(key), _bits(W.extraction_key(cov, s))), (name, route)
            assert np.array_equal(np.asarray(W.extract_watermark_keyed(img, key, s)), np.asarray(W.extract_watermark(img, cov, s))), name
    assert seen == set(BLOCKS)


def test_pipeline_return_keys(dev):
    from thatsmyface_amd import pipeline
    from thatsmyface_amd import watermarking as W

    s = {"block_size": 8, "alpha": 0.1}
    sizes = [(96, 64), (96, 64), (61, 37), (203, 139), (16, 8)]
    imgs = [Image.fromarray(_u8(80 + i, (h, w, 3))) for i, (w, h) in enumerate(sizes)]
    buf = io.BytesIO()
    Image.fromarray(_u8(90, (33, 33))).save(buf, format="PNG")
    wm = buf.getvalue()
    plain = pipeline.embed_images(imgs, wm, True, s)
    assert all(e.key is None for e in plain)
    for kw in ({}, {"batch_images": 3}):
        assert [e.png for e in pipeline.embed_images(imgs, wm, True, s, **kw)] == [e.png for e in plain]  # return_keys=False: unchanged
        res = pipeline.embed_images(imgs, wm, True, s, return_keys=True, **kw)
        for i, (img, e, p) in enumerate(zip(imgs, res, plain)):
            assert np.array_equal(e.pixels, p.pixels) and e.png == p.png, (kw, i)
            ref = W.extraction_key(img, s)
            assert e.key.dtype == np.float32 and e.key.shape == ref.shape and np.array_equal(_bits(e.key), _bits(ref)), (kw, i)
        # the verifier's side takes them as they are
        tiles = list(pipeline.extract_images([e.image() for e in res], [e.key for e in res], s))
        for i, (t, e) in enumerate(zip(tiles, res)):
            assert np.array_equal(np.asarray(t), np.asarray(W.extract_watermark(e.image(), imgs[i], s))), (kw, i)
