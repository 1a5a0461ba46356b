"""The ragged calls with one alpha per frame, on the GPU: batch.embed_ragged / embed_ragged_rank1 /
embed_with_key_ragged(_rank1) / extract_ragged / extract_keyed_ragged with alpha a sequence, the
four tmfwm_*_ragged_alphas entries through ctypes, and pipeline.embed_images / extract_images with
one settings dict per image.

The yardstick is always the single-frame call (batch.embed_batch / extract_batch / extract_keyed,
unchanged code) on that frame alone at that frame's alpha, byte for byte, and its counts summed;
for the mixed batch also the oracle's dgesdd route on the reference route.  The shapes are the
smallest at which a kernel of the per-frame form can take the wrong alpha: a frame whose block
rows end mid-wave next to a frame with another alpha, frames without a block between frames with
blocks, fixup waves that hold blocks of several frames, chunks that must use their own slice of
the alpha table, list-pass waves on the rank-1 route."""
import ctypes
import functools
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


def _tile(nbh, nbw, seed=7):
    n = nbh * nbw
    if n == 0:
        return np.zeros((nbh, nbw), np.uint8)
    return np.ascontiguousarray(((O.synth_bytes(0x5EED0002, seed, 1, n) & 1) * 255).astype(np.uint8).reshape(nbh, nbw))


def _photo(H, W, seed):
    from lapack_path import photo_cover

    if H == 0 or W == 0:
        return np.zeros((H, W, 3), np.uint8)
    return np.ascontiguousarray(photo_cover(H, W, seed))


def _dev(arrays, dev):
    return [torch.from_numpy(np.array(a)).to(dev) for a in arrays]  # (a copy: shared arrays are read only)


def _rgbx(t):
    """(H, W, 3) -> (H, W, 4) R G B pad, the pad byte not zero."""
    out = torch.full(t.shape[:2] + (4,), 0xA5, dtype=torch.uint8, device=t.device)
    out[..., :3] = t
    return out.contiguous()


def _bits(t):
    return t.view(torch.int32)


# ---- the mixed batch

def _mixed_shapes(b):
    # 35 blocks per row: strip waves end mid-row next to a frame with another alpha; a long frame; one
    # block; a small frame; no block; no pixel; and (the embeds' alpha 0.0) a frame of two blocks
    return [(3 * b + 3, 35 * b + 5), (4 * b, 64 * b), (b, b), (2 * b, 3 * b), (b - 1, 40), (b, 0), (b, 2 * b)]


def _mixed_alphas(b, embed):
    return [0.1, -0.5, 2.0, float(b), 1 / 3, 0.0 if embed else 0.7, 0.0 if embed else -0.25]


@functools.lru_cache(maxsize=None)
def _mixed(b):
    covers = [_photo(H, W, 13 + i) for i, (H, W) in enumerate(_mixed_shapes(b))]
    tiles = [_tile(H // b, W // b, 7 + i) for i, (H, W) in enumerate(_mixed_shapes(b))]
    for a in covers + tiles:
        a.setflags(write=False)
    return covers, tiles


_SINGLE = {}


def _single_embed(dev, b, route):
    """embed_batch on every frame of _mixed(b) alone at its alpha: (outputs, summed lapack_blocks, summed list_pass_blocks)."""
    from thatsmyface_amd import batch

    if (b, route) not in _SINGLE:
        covers, tiles = _mixed(b)
        outs, lap, lst = [], 0, 0
        for f, t, a in zip(_dev(covers, dev), _dev(tiles, dev), _mixed_alphas(b, True)):
            if f.numel() == 0:
                outs.append(f)
                continue
            st = {}
            outs.append(batch.embed_batch(f[None], t, b, a, stats=st, route=route)[0])
            lap += st["lapack_blocks"]
            lst += st["list_pass_blocks"]
        _SINGLE[(b, route)] = (outs, lap, lst)
    return _SINGLE[(b, route)]


def _check_embed(out, st, dev, b, route, extra=(0, 0)):
    covers, tiles = _mixed(b)
    souts, lap, lst = _single_embed(dev, b, route)
    assert len(out) == len(covers)
    for i, (o, s) in enumerate(zip(out, souts)):
        assert o.shape == s.shape and torch.equal(o, s), (b, route, i)
    if not route.startswith("rank1"):  # the single-size hybrid embed defers blocks to a list pass at b = 8, the ragged one has none
        lst = 0
    assert st == {"lapack_blocks": lap + extra[0], "list_pass_blocks": lst + extra[1]}, (b, route, st, lap, lst, extra)


@pytest.mark.parametrize("b", ALL_B)
def test_mixed_batch_embed(dev, b):
    from thatsmyface_amd import batch

    covers, tiles = _mixed(b)
    alphas = _mixed_alphas(b, True)
    fr, tt = _dev(covers, dev), _dev(tiles, dev)
    sm = {}
    kref = batch.sigma1_map_ragged(fr, b, stats=sm)
    routes = ("hybrid", "reference") + (("rank1", "rank1_reference") if b in (8, 12) else ())
    for route in routes:
        rank1 = route.startswith("rank1")
        st = {}
        out = (batch.embed_ragged_rank1 if rank1 else batch.embed_ragged)(fr, tt, b, alphas, stats=st, route=route)
        _check_embed(out, st, dev, b, route)
        if not rank1:  # the other function, the same entry
            s2 = {}
            out2 = batch.embed_ragged_rank1(fr, tt, b, tuple(alphas), stats=s2, route=route)
            _check_embed(out2, s2, dev, b, route)
        sk = {}
        kout, keys = (batch.embed_with_key_ragged_rank1 if rank1 else batch.embed_with_key_ragged)(fr, tt, b, alphas, stats=sk, route=route)
        # on a rank-1 route the key call is composed: the map's counts on top of the embed's
        _check_embed(kout, sk, dev, b, route, extra=(sm["lapack_blocks"], sm["list_pass_blocks"]) if rank1 else (0, 0))
        for i, (k, r) in enumerate(zip(keys, kref)):  # the key bits do not depend on alpha
            assert k.shape == r.shape and torch.equal(_bits(k), _bits(r)), (b, route, i)
    # the oracle's dgesdd route, per frame at its alpha
    souts, _, _ = _single_embed(dev, b, "reference")
    for i, (c, t, a) in enumerate(zip(covers, tiles, alphas)):
        if t.size:
            assert np.array_equal(souts[i].cpu().numpy(), O.embed_frame(c, t, b, a, route="lapack")), (b, i)


@pytest.mark.parametrize("b", ALL_B)
def test_mixed_batch_extract(dev, b):
    from thatsmyface_amd import batch

    covers, tiles = _mixed(b)
    alphas = _mixed_alphas(b, False)
    fr, tt = _dev(covers, dev), _dev(tiles, dev)
    wm = batch.embed_ragged(fr, tt, b, alphas)  # (its bytes are test_mixed_batch_embed's business)
    keys = batch.sigma1_map_ragged(fr, b)
    wm4 = [_rgbx(w) for w in wm]
    for route in ("hybrid", "reference"):
        pair, keyed, lap_p, lap_k = [], [], 0, 0
        for w, o, k, a in zip(wm, fr, keys, alphas):
            if k.numel() == 0:
                pair.append(None)
                keyed.append(None)
                continue
            s1, s2 = {}, {}
            pair.append(batch.extract_batch(w[None], o[None], b, a, stats=s1, route=route)[0])
            keyed.append(batch.extract_keyed(w[None], k, b, a, stats=s2, route=route)[0])
            lap_p += s1["lapack_blocks"]
            lap_k += s2["lapack_blocks"]
        sp, sk, s4 = {}, {}, {}
        got_p = batch.extract_ragged(wm, fr, b, alphas, stats=sp, route=route)
        got_k = batch.extract_keyed_ragged(wm, keys, b, alphas, stats=sk, route=route)
        got_4 = batch.extract_keyed_ragged(wm4, keys, b, alphas, stats=s4, route=route)
        assert sp == {"lapack_blocks": lap_p, "list_pass_blocks": 0} and sk == s4 == {"lapack_blocks": lap_k, "list_pass_blocks": 0}, \
            (b, route, sp, sk, s4, lap_p, lap_k)
        for i in range(len(fr)):
            assert got_p[i].shape == got_k[i].shape == got_4[i].shape == tiles[i].shape, (b, route, i)
            if pair[i] is None:
                continue
            assert torch.equal(got_p[i], pair[i]), (b, route, i)
            assert torch.equal(got_k[i], keyed[i]) and torch.equal(got_4[i], keyed[i]), (b, route, i)
            if route == "reference":
                want = O.extract_frame(wm[i].cpu().numpy(), covers[i], b, alphas[i], route="lapack")
                assert np.array_equal(got_p[i].cpu().numpy(), want), (b, i)
                assert np.array_equal(got_k[i].cpu().numpy(), want), (b, i)


# ---- fixup waves across frames

@pytest.mark.parametrize("b", (4, 8, 16))
def test_fixup_waves_hold_several_frames(dev, b):
    """24 frames of one to four blocks on the reference route, 24 distinct alphas: every block is on
    the dgesdd route, whose waves take blocks off the list whatever their frame, so a wave-uniform
    alpha in a fixup kernel shows here."""
    from thatsmyface_amd import batch

    rng = np.random.default_rng(2400 + b)
    shapes = [(int(rng.integers(b, 2 * b + 1)), int(rng.integers(b, 2 * b + 1))) for _ in range(24)]
    shapes[3], shapes[17] = (2 * b, 2 * b), (b, b)
    alphas = [(0.04 * (i + 1)) * (-1 if i % 5 == 2 else 1) for i in range(24)]
    assert len(set(alphas)) == 24
    big = _photo(4 * b, 6 * b, 31)
    covers = [np.ascontiguousarray(big[i % (2 * b):][:H, (3 * i) % (4 * b):][:, :W]) for i, (H, W) in enumerate(shapes)]
    assert all(c.shape[:2] == s for c, s in zip(covers, shapes))
    tiles = [_tile(H // b, W // b, 50 + i) for i, (H, W) in enumerate(shapes)]
    blocks = sum(t.size for t in tiles)
    fr, tt = _dev(covers, dev), _dev(tiles, dev)
    st = {}
    wm = batch.embed_ragged(fr, tt, b, alphas, stats=st, route="reference")
    assert st == {"lapack_blocks": blocks, "list_pass_blocks": 0}, (st, blocks)
    keys = batch.sigma1_map_ragged(fr, b)
    sp, sk = {}, {}
    got_p = batch.extract_ragged(wm, fr, b, alphas, stats=sp, route="reference")
    got_k = batch.extract_keyed_ragged(wm, keys, b, alphas, stats=sk, route="reference")
    assert sp["lapack_blocks"] == blocks and sk["lapack_blocks"] == blocks, (sp, sk, blocks)
    for i, a in enumerate(alphas):
        assert torch.equal(wm[i], batch.embed_batch(fr[i][None], tt[i], b, a, route="reference")[0]), (b, i)
        assert torch.equal(got_p[i], batch.extract_batch(wm[i][None], fr[i][None], b, a, route="reference")[0]), (b, i)
        assert torch.equal(got_k[i], batch.extract_keyed(wm[i][None], keys[i], b, a, route="reference")[0]), (b, i)


# ---- chunks

def test_chunks_use_their_own_slice_of_the_alpha_table(dev, monkeypatch):
    """TMFWM_DEBUG_LIST_CAP at 1.5 frames' worth of ids (as tests/test_keyed_gpu.py sets it): four
    frames with four alphas are four chunks; bytes and counts are the unchunked call's."""
    from keyed_helpers import sparks

    from thatsmyface_amd import batch

    b, H, W = 8, 64, 128
    nb = (H // b) * (W // b)
    covers = [_photo(H, W, 30), sparks(H, W, b, 31), _photo(H, W, 32), sparks(H, W, b, 33)]
    alphas = [0.1, 0.35, -0.5, 1.5]
    fr, tt = _dev(covers, dev), _dev([_tile(H // b, W // b, 60 + i) for i in range(4)], dev)

    def run():
        se, sk, sx, sp = {}, {}, {}, {}
        wm = batch.embed_ragged(fr, tt, b, alphas, stats=se)
        wm2, keys = batch.embed_with_key_ragged(fr, tt, b, alphas, stats=sk)
        tiles = batch.extract_keyed_ragged(wm, keys, b, alphas, stats=sx)
        pairs = batch.extract_ragged(wm, fr, b, alphas, stats=sp)
        return (wm, wm2, tiles, pairs), (se, sk, sx, sp)

    t0, s0 = run()
    monkeypatch.setenv("TMFWM_DEBUG_LIST_CAP", str(nb * 3 // 2))
    t1, s1 = run()
    monkeypatch.delenv("TMFWM_DEBUG_LIST_CAP")
    assert s0 == s1, (s0, s1)
    assert s0[2]["lapack_blocks"] >= 2 * nb, s0  # the sparks frames' blocks: every chunk's fixup pass ran
    for x, y in zip(t0, t1):
        for i in range(4):
            assert torch.equal(x[i], y[i]), i
    for i, a in enumerate(alphas):
        w = batch.embed_batch(fr[i][None], tt[i], b, a)
        assert torch.equal(t1[0][i], w[0]) and torch.equal(t1[1][i], w[0]), i
        assert torch.equal(t1[2][i], batch.extract_batch(w, fr[i][None], b, a)[0]), i
        assert torch.equal(t1[3][i], t1[2][i]), i


# ---- the rank-1 routes

@pytest.mark.parametrize("b", (8, 12))
def test_rank1_routes(dev, b):
    """Photographs (rank1_classes' covers) of mixed sizes, each at its own alpha: the pre-pass keeps
    some blocks of every frame and leaves some to the list pass -- asserted on the single-frame
    calls' numbers -- so both the pre-pass and the list pass read the per-frame alpha."""
    import rank1_classes

    from thatsmyface_amd import batch

    shapes = [(5 * b, 7 * b + 2), (3 * b + 3, 9 * b + 1), (6 * b, 4 * b), (b - 1, 3 * b), (4 * b, 6 * b)]
    alphas = [0.1, 1.0, -0.5, 0.2, 0.05]
    covers = [np.ascontiguousarray(rank1_classes.photo_cover(H, W, rank1_classes.PHOTO_SEEDS[i])) for i, (H, W) in enumerate(shapes)]
    tiles = [_tile(H // b, W // b, 70 + i) for i, (H, W) in enumerate(shapes)]
    fr, tt = _dev(covers, dev), _dev(tiles, dev)
    ref = batch.embed_ragged(fr, tt, b, alphas, route="reference")
    for route in ("rank1", "rank1_reference"):
        left = "list_pass_blocks" if route == "rank1" else "lapack_blocks"
        lap = lst = 0
        for i, a in enumerate(alphas):
            s1 = {}
            one = batch.embed_batch(fr[i][None], tt[i], b, a, stats=s1, route=route)[0]
            assert torch.equal(one, ref[i]), (b, route, i)
            if tiles[i].size:  # the precondition: blocks kept and blocks left, frame by frame
                assert 0 < s1[left] < tiles[i].size, (b, route, i, s1, tiles[i].size)
            lap += s1["lapack_blocks"]
            lst += s1["list_pass_blocks"]
        st = {}
        out = batch.embed_ragged_rank1(fr, tt, b, alphas, stats=st, route=route)
        assert st == {"lapack_blocks": lap, "list_pass_blocks": lst}, (b, route, st, lap, lst)
        for i in range(len(fr)):
            assert torch.equal(out[i], ref[i]), (b, route, i)


# ---- one input, several alphas

def test_strength_sweep_shares_its_input(dev):
    from thatsmyface_amd import batch

    b = 8
    f = _dev([_photo(5 * b, 9 * b + 3, 21)], dev)[0]
    t = _dev([_tile(5, 9)], dev)[0]
    alphas = [0.02, 0.05, 0.1, 0.2, 0.5, 1.0, -0.1, 0.0]
    for route in ("hybrid", "rank1"):
        out = (batch.embed_ragged_rank1 if route == "rank1" else batch.embed_ragged)([f] * 8, [t] * 8, b, alphas, route=route)
        assert len({o.data_ptr() for o in out}) == 8
        for o, a in zip(out, alphas):
            assert torch.equal(o, batch.embed_batch(f[None], t, b, a, route=route)[0]), (route, a)


# ---- host memory through the C entries

def _desc(kind, rows):
    arr = (kind * len(rows))()
    for i, r in enumerate(rows):
        arr[i] = kind(*r)
    return arr


def test_host_memory_through_the_c_entries(dev):
    from thatsmyface_amd import _lib, batch

    L = _lib.load()
    b = 6
    covers, tiles = _mixed(b)
    n = len(covers)
    alphas = _mixed_alphas(b, True)
    souts, lap, _ = _single_embed(dev, b, "hybrid")
    CAN = 32
    outs = [np.full(c.size + 2 * CAN, 0xC3, np.uint8) for c in covers]
    rows = [(c.ctypes.data if c.size else None, o.ctypes.data + CAN, t.ctypes.data if t.size else None, c.shape[0], c.shape[1])
            for c, o, t in zip(covers, outs, tiles)]
    d = _desc(_lib.EmbedFrame, rows)
    arr = (ctypes.c_double * n)(*alphas)
    cnt = ctypes.c_int64(-1)
    _lib.check(L.tmfwm_embed_ragged_alphas(ctypes.addressof(d), ctypes.addressof(arr), n, b, _lib.MEM_HOST, None, _lib.ROUTE_HYBRID,
                                           ctypes.addressof(cnt)), "embed_ragged_alphas")
    assert cnt.value == lap
    for i, (o, c) in enumerate(zip(outs, covers)):
        assert np.array_equal(o[CAN:len(o) - CAN].reshape(c.shape), souts[i].cpu().numpy()), i
        assert (o[:CAN] == 0xC3).all() and (o[len(o) - CAN:] == 0xC3).all(), i
    # the keyed extract from those outputs as 4-byte pixels
    xa = _mixed_alphas(b, False)
    wms = [np.ascontiguousarray(_rgbx(s).cpu().numpy()) if s.numel() else np.zeros(s.shape[:2] + (4,), np.uint8) for s in souts]
    keys = [k.cpu().numpy() for k in batch.sigma1_map_ragged(_dev(covers, dev), b)]
    touts = [np.full(t.size + 2 * CAN, 0xC3, np.uint8) for t in tiles]
    rows = [(w.ctypes.data if t.size else None, k.ctypes.data if t.size else None, o.ctypes.data + CAN if t.size else None, c.shape[0],
             c.shape[1]) for w, k, o, t, c in zip(wms, keys, touts, tiles, covers)]
    d = _desc(_lib.KeyedFrame, rows)
    arr = (ctypes.c_double * n)(*xa)
    cnt = ctypes.c_int64(-1)
    _lib.check(L.tmfwm_extract_keyed_ragged_alphas(ctypes.addressof(d), ctypes.addressof(arr), n, b, 4, _lib.MEM_HOST, None,
                                                   _lib.ROUTE_HYBRID, ctypes.addressof(cnt)), "extract_keyed_ragged_alphas")
    fr = _dev(covers, dev)
    lap_k = 0
    for i, (o, t) in enumerate(zip(touts, tiles)):
        assert (o[:CAN] == 0xC3).all() and (o[len(o) - CAN:] == 0xC3).all(), i
        if not t.size:
            continue
        s1 = {}
        want = batch.extract_batch(souts[i][None], fr[i][None], b, xa[i], stats=s1)[0].cpu().numpy()
        sk = {}
        batch.extract_keyed(souts[i][None], torch.from_numpy(keys[i]).to(dev), b, xa[i], stats=sk)
        lap_k += sk["lapack_blocks"]
        assert np.array_equal(o[CAN:len(o) - CAN].reshape(t.shape), want), i
    assert cnt.value == lap_k


# ---- the pipeline

def test_pipeline_per_image_settings(dev):
    """Six images, two block sizes and four alphas, in groups of four: embed_images and
    extract_images against the drop-ins called image by image with that image's settings."""
    from PIL import Image

    from thatsmyface_amd import pipeline
    from thatsmyface_amd import watermarking as W

    shapes = [(96, 128), (60, 90), (96, 128), (64, 100), (33, 47), (80, 64)]
    settings = [{"block_size": 8, "alpha": 0.1}, {"block_size": 4, "alpha": 0.25}, {"block_size": 8, "alpha": 0.4},
                {"block_size": 4, "alpha": 0.1}, {"block_size": 8, "alpha": 0.05, "svd_route": "hybrid"}, {"block_size": 4, "alpha": 0.4}]
    imgs, wms = [], []
    for k, (H, W_) in enumerate(shapes):
        arr = _photo(H, W_, 80 + k)
        buf = io.BytesIO()
        Image.fromarray(arr).save(buf, format="PNG")
        imgs.append(buf.getvalue() if k % 2 else Image.fromarray(arr))
        wms.append(Image.fromarray(((O.synth_bytes(0x5EED0002, 20 + k, 1, 29 * 29) & 1) * 255).astype(np.uint8).reshape(29, 29), "L"))

    def pil(src):
        return src if isinstance(src, Image.Image) else Image.open(io.BytesIO(src))

    grp = pipeline.embed_images(imgs, wms, True, settings, batch_images=4, return_keys=True)
    plain = pipeline.embed_images(imgs, wms, True, tuple(settings), batch_images=4)
    one = pipeline.embed_images(imgs, wms, True, settings)
    assert len(grp) == len(plain) == len(one) == 6
    for i, s in enumerate(settings):
        want = np.asarray(W.embed_watermark(pil(imgs[i]), wms[i], True, s).convert("RGB"))
        for r in (grp[i], plain[i], one[i]):
            assert np.array_equal(r.pixels, want), i
            assert np.array_equal(np.asarray(Image.open(io.BytesIO(r.png))), want), i
        assert np.array_equal(grp[i].key.view(np.uint32), W.extraction_key(pil(imgs[i]), s).view(np.uint32)), i
    got = list(pipeline.extract_images([g.png if i % 2 else g.image() for i, g in enumerate(grp)], [g.key for g in grp], settings,
                                       batch_images=4))
    for i, (g, e) in enumerate(zip(got, grp)):
        want = W.extract_watermark_keyed(e.image(), e.key, settings[i])
        assert g.size == want.size and np.array_equal(np.asarray(g), np.asarray(want)), i
