"""Ragged tile preparation on the GPU: batch.prepare_tiles_ragged, tmfwm_prepare_tiles_ragged
through ctypes, and the batched pipeline stage that prepares a group's tiles with it.

Every tile has two yardsticks: the oracle's prepare_tile, and batch.prepare_tile (unchanged entry
point) called for that job alone.  The job list and its index paths: tests/tiles_ragged_jobs.py;
the same list runs through the plan and both passes on the host in tests/test_tiles_ragged.py."""
import ctypes
import io

import numpy as np
import pytest

from oracle import oracle as O
from tiles_ragged_jobs import ERROR_JOBS, JOBS, expected, watermarks

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FRAMES = [(48, 64), (40, 56), (64, 48)]  # the three small frames of the stream-order and pipeline tests, b = 8


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from thatsmyface_amd import _lib

    assert _lib.device_count() > 0
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def wms(dev):
    return [torch.from_numpy(w).to(dev) for w in watermarks()]


@pytest.fixture(scope="module")
def single(dev, wms):
    """batch.prepare_tile of every job alone, per preserve_ratio (computed once, left unchanged)."""
    from thatsmyface_amd import batch

    return {pr: [batch.prepare_tile(w, th, tw, pr) for w, (_, (th, tw)) in zip(wms, JOBS)] for pr in (False, True)}


def _padded_views(dev):
    """Tiles of list J as views of one 0x5A buffer with odd gaps -> (buffer, views, mask of tile bytes)."""
    offs, o = [], 0
    for i, (_, (th, tw)) in enumerate(JOBS):
        o += 5 + 3 * i
        offs.append(o)
        o += th * tw
    buf = torch.full((o + 11,), 0x5A, dtype=torch.uint8, device=dev)
    mask = torch.zeros(o + 11, dtype=torch.bool, device=dev)
    views = []
    for off, (_, (th, tw)) in zip(offs, JOBS):
        views.append(buf[off:off + th * tw].view(th, tw))
        mask[off:off + th * tw] = True
    return buf, views, mask


def _check(tiles, preserve, single, what):
    want = expected(preserve)
    for i, t in enumerate(tiles):
        assert tuple(t.shape) == JOBS[i][1]
        assert np.array_equal(t.cpu().numpy(), want[i]), (what, preserve, i, JOBS[i])
        assert torch.equal(t, single[preserve][i]), (what, preserve, i, JOBS[i])


@pytest.mark.parametrize("preserve", [False, True])
def test_list_j_device_memory(dev, wms, single, preserve):
    from thatsmyface_amd import batch

    sizes = [t for _, t in JOBS]
    buf, views, mask = _padded_views(dev)
    got = batch.prepare_tiles_ragged(wms, sizes, preserve, out=views)
    assert all(g is v for g, v in zip(got, views))
    _check(got, preserve, single, "out=")
    assert (buf[~mask] == 0x5A).all(), "a byte outside the tiles was written"
    assert not torch.equal(got[2], got[3])  # one plan, two data sets
    own = batch.prepare_tiles_ragged(wms, sizes, preserve)  # views of one allocation of the call's own
    assert len({t.data_ptr() for t in own}) == len(own)
    assert len({t.untyped_storage().data_ptr() for t in own}) == 1
    _check(own, preserve, single, "own")
    assert batch.prepare_tiles_ragged([], [], preserve) == []
    with pytest.raises(ValueError, match="out"):
        batch.prepare_tiles_ragged(wms, sizes, preserve, out=views[:-1])
    with pytest.raises(ValueError, match="out"):
        batch.prepare_tiles_ragged(wms, sizes, preserve, out=views[1:] + views[:1])


def _desc(rows):
    from thatsmyface_amd import _lib

    d = (_lib.TileJob * len(rows))()
    for i, r in enumerate(rows):
        d[i] = _lib.TileJob(*r)
    return d


def test_list_j_host_memory(dev, single):
    from thatsmyface_amd import _lib

    L = _lib.load()
    for preserve in (False, True):
        hw = [np.ascontiguousarray(w) for w in watermarks()]
        tiles = [np.full(t, 0x5A, np.uint8) for _, t in JOBS]
        d = _desc([(w.ctypes.data, t.ctypes.data, w.shape[0], w.shape[1], t.shape[0], t.shape[1]) for w, t in zip(hw, tiles)])
        _lib.check(L.tmfwm_prepare_tiles_ragged(ctypes.addressof(d), len(JOBS), int(preserve), _lib.MEM_HOST, None), "host")
        for i, (t, w) in enumerate(zip(tiles, expected(preserve))):
            assert np.array_equal(t, w), (preserve, i, JOBS[i])


def test_one_shared_watermark(dev, wms):
    """One watermark tensor for every size: the inputs alias."""
    from thatsmyface_amd import batch

    sizes = [(2, 3), (17, 25), (60, 80), (60, 80), (300, 300), (38, 51), (135, 240)]
    w = wms[1]
    for preserve in (False, True):
        got = batch.prepare_tiles_ragged(w, sizes, preserve)
        for i, (t, (th, tw)) in enumerate(zip(got, sizes)):
            assert np.array_equal(t.cpu().numpy(), O.prepare_tile(watermarks()[1], th, tw, preserve)), (preserve, i)
            assert torch.equal(t, batch.prepare_tile(w, th, tw, preserve)), (preserve, i)


def test_groups(dev, wms, single, monkeypatch):
    """TMFWM_DEBUG_TILE_SCRATCH bounds a group's scratch: 8000 bytes cut list J into several
    groups (the two 300 x 80 jobs alone exceed it), 1 byte starts a group at every job with a
    horizontal pass; the groups share one scratch in stream order and the bytes do not change."""
    from thatsmyface_amd import batch

    sizes = [t for _, t in JOBS]
    for cap in (8000, 1):
        monkeypatch.setenv("TMFWM_DEBUG_TILE_SCRATCH", str(cap))
        for preserve in (False, True):
            buf, views, mask = _padded_views(dev)
            _check(batch.prepare_tiles_ragged(wms, sizes, preserve, out=views), preserve, single, f"cap {cap}")
            assert (buf[~mask] == 0x5A).all()


def test_stream_order_with_embed_ragged(dev):
    """prepare_tiles_ragged and then embed_ragged on a side stream with no synchronisation between
    them, the descriptor list overwritten right after the call returned."""
    from thatsmyface_amd import _lib, batch

    b, alpha = 8, 0.1
    rng = np.random.default_rng(81)
    covers = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in FRAMES]
    grey = [(rng.integers(0, 2, (300, 300)) * 255).astype(np.uint8) for _ in FRAMES]
    fr = [torch.from_numpy(c).to(dev) for c in covers]
    gw = [torch.from_numpy(g).to(dev) for g in grey]
    tiles = [torch.full((h // b, w // b), 7, dtype=torch.uint8, device=dev) for h, w in FRAMES]
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    L = _lib.load()
    with torch.cuda.stream(side):
        d = _desc([(g.data_ptr(), t.data_ptr(), 300, 300, t.shape[0], t.shape[1]) for g, t in zip(gw, tiles)])
        _lib.check(L.tmfwm_prepare_tiles_ragged(ctypes.addressof(d), 3, 1, _lib.MEM_DEVICE, side.cuda_stream), "prepare_tiles_ragged")
        ctypes.memset(ctypes.addressof(d), 0xA5, ctypes.sizeof(d))  # the call has returned: the array is the caller's again
        out = batch.embed_ragged(fr, tiles, b, alpha, stream=side)
    side.synchronize()
    for i, (h, w) in enumerate(FRAMES):
        t = O.prepare_tile(grey[i], h // b, w // b, True)
        assert np.array_equal(tiles[i].cpu().numpy(), t), i
        assert np.array_equal(out[i].cpu().numpy(), O.embed_frame(covers[i], t, b, alpha)), i


def test_refusals(dev, wms):
    from thatsmyface_amd import _lib

    L = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    big = torch.full((4096,), 0x5A, dtype=torch.uint8, device=dev)
    w = wms[4]  # 29 x 31

    def call(rows, preserve=0):
        d = _desc(rows)
        return L.tmfwm_prepare_tiles_ragged(ctypes.addressof(d), len(rows), preserve, _lib.MEM_DEVICE, stream)

    ok = [(w.data_ptr(), big.data_ptr(), 29, 31, 17, 25), (w.data_ptr(), big.data_ptr() + 1000, 29, 31, 20, 31)]
    assert call(ok) == 0, _lib.last_error()
    # a tile inside a watermark of the call (another job's), and two tiles that share bytes
    assert call([ok[0], (wms[5].data_ptr(), w.data_ptr() + 100, 29, 31, 5, 5)]) == _lib.ERR_INVALID
    assert "overlaps" in _lib.last_error()
    assert call([ok[0], (w.data_ptr(), big.data_ptr() + 17 * 25 - 1, 29, 31, 20, 31)]) == _lib.ERR_INVALID
    assert "overlaps" in _lib.last_error()
    host = np.zeros((29, 31), np.uint8)  # a host pointer handed in as device memory
    assert call([ok[0], (host.ctypes.data, big.data_ptr() + 1000, 29, 31, 20, 31)]) == _lib.ERR_INVALID
    assert "not" in _lib.last_error() and "job 1" in _lib.last_error(), _lib.last_error()
    torch.cuda.synchronize()
    big.fill_(0x5A)
    torch.cuda.synchronize()
    # the error jobs under preserve_ratio: refused by index, and no tile of the call is written
    for k, ((wh, ww), (th, tw)) in enumerate(ERROR_JOBS):
        thin = torch.zeros((wh, ww), dtype=torch.uint8, device=dev)
        rows = [ok[0], ok[1], (thin.data_ptr(), big.data_ptr() + 2000, wh, ww, th, tw)]
        assert call(rows, preserve=1) == _lib.ERR_INVALID
        assert "job 2" in _lib.last_error(), _lib.last_error()
        torch.cuda.synchronize()
        assert (big == 0x5A).all(), k
        assert call(rows, preserve=0) == 0, _lib.last_error()  # valid without it
        torch.cuda.synchronize()
        assert np.array_equal(big[2000:2000 + th * tw].view(th, tw).cpu().numpy(), O.prepare_tile(np.zeros((wh, ww), np.uint8), th, tw, False))
        big.fill_(0x5A)
        torch.cuda.synchronize()


def test_pipeline_prepares_a_group_with_one_ragged_call(dev, monkeypatch):
    """Six images in three sizes, six distinct watermarks, groups of four: the stage never calls
    prepare_tile / prepare_tiles, and pixels and PNG bytes are the per-image oracle result; then
    one shared watermark."""
    from PIL import Image

    from thatsmyface_amd import batch, pipeline
    from thatsmyface_amd.constants import SVD_ROUTE

    def refuse(*a, **k):
        raise AssertionError("the batched stage prepared a tile on its own")

    monkeypatch.setattr(batch, "prepare_tile", refuse)
    monkeypatch.setattr(batch, "prepare_tiles", refuse)
    calls = []
    real = batch.prepare_tiles_ragged
    monkeypatch.setattr(batch, "prepare_tiles_ragged", lambda w, s, *a, **k: (calls.append(len(s)), real(w, s, *a, **k))[1])
    b, alpha = 8, 0.15
    rng = np.random.default_rng(91)
    covers = [rng.integers(0, 256, (*FRAMES[i % 3], 3), dtype=np.uint8) for i in range(6)]
    grey = [(rng.integers(0, 2, (29, 29)) * 255).astype(np.uint8) for _ in range(6)]
    imgs = [Image.fromarray(c) for c in covers]
    wms = [Image.fromarray(g, "L") for g in grey]
    route = {"reference": "lapack", "hybrid": None}[SVD_ROUTE]

    def oracle(i, g):
        h, w = covers[i].shape[:2]
        return O.embed_frame(covers[i], O.prepare_tile(g, h // b, w // b, True), b, alpha, route=route)

    res = pipeline.embed_images(imgs, wms, True, {"block_size": b, "alpha": alpha}, batch_images=4)
    assert calls == [4, 2]  # one call per group, a key per image
    for i, r in enumerate(res):
        ref = oracle(i, grey[i])
        assert np.array_equal(r.pixels, ref), i
        buf = io.BytesIO()
        Image.fromarray(ref, "RGB").save(buf, format="PNG")
        assert r.png == buf.getvalue(), i
    calls.clear()
    res = pipeline.embed_images(imgs, wms[0], True, {"block_size": b, "alpha": alpha}, batch_images=4)
    assert calls == [3]  # three sizes in the first group, cached for the second
    for i, r in enumerate(res):
        ref = oracle(i, grey[0])
        assert np.array_equal(r.pixels, ref), i
        buf = io.BytesIO()
        Image.fromarray(ref, "RGB").save(buf, format="PNG")
        assert r.png == buf.getvalue(), i
