"""The ragged embed on the rank-1 routes, on the GPU: batch.embed_ragged_rank1 /
embed_with_key_ragged_rank1, tmfwm_embed_ragged_rank1 / tmfwm_embed_key_ragged_rank1 through
ctypes, and pipeline.embed_images / extract_images with batch_images on those routes.

Every frame of a call has two yardsticks: the oracle's dgesdd route on that frame (every route
gives the reference's bytes) and the single-size path (batch.embed_batch, unchanged code) on that
frame alone on the same route, whose counts the ragged call's must sum to.  The frames are the
smallest at which the kernels can go wrong: edges on both sides, a block row longer than one strip
wave, a frame without a block, a skipped frame, a frame whose every block the pre-pass's gate
refuses (sparks) and one whose every block it keeps (black); rank1_classes.classify on these very
frames says, on the CPU, how many blocks the pre-pass must keep and must leave, so that no test
passes with one path unrun.
"""
import ctypes
import functools
import io

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ALL_B = (4, 6, 8, 10, 12, 14, 16)
RANK1 = ("rank1", "rank1_reference")
ALPHA = 0.1


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from thatsmyface_amd import _lib

    assert _lib.device_count() > 0
    return torch.device("cuda", 0)


def _bpw(b):
    return 64 // (1 if b == 4 else 2 if b <= 8 else 4 if b <= 12 else 8)  # Geo<b>::BPW


def _tile(nbh, nbw):
    n = nbh * nbw
    if n == 0:
        return np.zeros((nbh, nbw), np.uint8)
    return np.ascontiguousarray(((O.synth_bytes(0x5EED0002, 7, 1, n) & 1) * 255).astype(np.uint8).reshape(nbh, nbw))


def _cover(kind, H, W, b):
    from keyed_helpers import sparks
    from lapack_path import photo_cover

    if kind == "photo":
        return np.ascontiguousarray(photo_cover(H, W, 13))
    if kind == "sparks":
        return sparks(H, W, b, 41)
    return np.zeros((H, W, 3), np.uint8)


def _shapes(b):
    return [("photo", 3 * b + 3, 5 * b + 1), ("photo", 2 * b, (_bpw(b) + 1) * b), ("photo", 5 * b, 7 * b + 2), ("photo", b - 1, 9 * b),
            ("black", 0, 7), ("sparks", 3 * b, 4 * b), ("black", 2 * b, 3 * b)]


SPARKS, BLACK = 5, 6  # their places in _shapes


@functools.lru_cache(maxsize=None)
def _case(b):
    """The frames of block size b, read only: covers, tiles, the oracle's outputs, and per frame the
    (must-refuse, must-accept, blocks) counts of rank1_classes.classify."""
    import rank1_classes

    covers, tiles, refs, counts = [], [], [], []
    for kind, H, W in _shapes(b):
        c, t = _cover(kind, H, W, b), _tile(H // b, W // b)
        covers.append(c)
        tiles.append(t)
        if t.size:
            refs.append(O.embed_frame(c, t, b, ALPHA, route="lapack"))
            r = rank1_classes.classify(c, t, b, ALPHA)
            counts.append((int(r["refuse"].sum()), int(r["accept"].sum()), t.size))
        else:
            refs.append(None)
            counts.append((0, 0, 0))
    # the precondition: each photo frame with blocks holds blocks of both kinds, the sparks frame
    # only blocks the pre-pass must leave, the black frame only blocks it must keep
    for i in range(3):
        refuse, accept, n = counts[i]
        assert refuse >= 1 and accept >= 1 and n - refuse - accept <= 1, (b, i, counts[i])
    assert counts[SPARKS] == (12, 0, 12) and counts[BLACK] == (0, 6, 6), (b, counts)
    for a in covers + tiles:
        a.setflags(write=False)
    return covers, tiles, refs, counts


def _dev(arrays, dev):
    return [torch.from_numpy(np.array(a)).to(dev) for a in arrays]  # (a copy: the shared arrays are read only)


_SINGLE = {}


def _single(dev, b, route):
    """The single-size path on every frame of _case(b) alone: (outputs as numpy, summed lapack_blocks, summed list_pass_blocks)."""
    from thatsmyface_amd import batch

    if (b, route) not in _SINGLE:
        covers, tiles, _, _ = _case(b)
        outs, lap, lst = [], 0, 0
        for f, t in zip(_dev(covers, dev), _dev(tiles, dev)):
            if f.numel() == 0:
                outs.append(np.zeros(f.shape, np.uint8))
                continue
            st = {}
            outs.append(batch.embed_batch(f[None], t, b, ALPHA, stats=st, route=route)[0].cpu().numpy())
            lap += st["lapack_blocks"]
            lst += st["list_pass_blocks"]
        _SINGLE[(b, route)] = (outs, lap, lst)
    return _SINGLE[(b, route)]


def _check_outputs(out, b, dev, route, order=None):
    covers, _, refs, _ = _case(b)
    souts, _, _ = _single(dev, b, route)
    for k, i in enumerate(order if order is not None else range(len(covers))):
        got = out[k].cpu().numpy() if isinstance(out[k], torch.Tensor) else out[k]
        assert got.shape == covers[i].shape, (b, route, i)
        assert np.array_equal(got, souts[i]), (b, route, i)
        if refs[i] is not None:
            assert np.array_equal(got, refs[i]), (b, route, i)


def _bounds(counts, frames):
    lo = sum(counts[i][0] for i in frames)
    hi = sum(counts[i][2] - counts[i][1] for i in frames)
    return lo, hi


@pytest.mark.parametrize("route", RANK1)
@pytest.mark.parametrize("b", ALL_B)
def test_bytes_and_counts(dev, b, route):
    from thatsmyface_amd import batch

    covers, tiles, _, counts = _case(b)
    fr, tt = _dev(covers, dev), _dev(tiles, dev)
    st = {}
    out = batch.embed_ragged_rank1(fr, tt, b, ALPHA, stats=st, route=route)
    _, lap, lst = _single(dev, b, route)
    print("stats", b, route, st, "single-size sums", lap, lst, "classes", counts)
    _check_outputs(out, b, dev, route)
    assert st == {"lapack_blocks": lap, "list_pass_blocks": lst}, (st, lap, lst)
    left = "list_pass_blocks" if route == "rank1" else "lapack_blocks"
    lo, hi = _bounds(counts, range(len(covers)))
    assert lo <= st[left] <= hi, (st, lo, hi)
    if route == "rank1_reference":
        assert st["list_pass_blocks"] == 0
    # the sparks frame alone leaves every block, the black frame alone none
    for i, want in ((SPARKS, counts[SPARKS][2]), (BLACK, 0)):
        s1 = {}
        o1 = batch.embed_ragged_rank1([fr[i]], [tt[i]], b, ALPHA, stats=s1, route=route)
        assert s1[left] == want, (i, s1)
        _check_outputs(o1, b, dev, route, order=[i])


def _chunks(blocks, cap):
    """The chunks the C ABI cuts frames of `blocks` blocks into (frames with nothing to do left out)."""
    out, cur = [], []
    for i, n in enumerate(blocks):
        if cur and sum(blocks[j] for j in cur) + n > cap:
            out.append(cur)
            cur = []
        cur.append(i)
    return out + [cur]


@pytest.mark.parametrize("route", RANK1)
@pytest.mark.parametrize("b", ALL_B)
def test_several_chunks(dev, monkeypatch, b, route):
    from thatsmyface_amd import batch

    covers, tiles, _, counts = _case(b)
    order = [0, 3, 2, 1, 5, 6, 4]  # 15 blocks, none | 35 | 2 (BPW + 1) >= 18 | 12, 6; the skipped frame last
    cap = 36
    chunks = _chunks([counts[i][2] for i in order[:-1]], cap)
    assert len(chunks) >= 3 and chunks[0] == [0, 1] and chunks[1] == [2], chunks  # a cut behind the no-block frame, one between frames with blocks
    monkeypatch.setenv("TMFWM_DEBUG_LIST_CAP", str(cap))
    fr, tt = _dev([covers[i] for i in order], dev), _dev([tiles[i] for i in order], dev)
    st = {}
    out = batch.embed_ragged_rank1(fr, tt, b, ALPHA, stats=st, route=route)
    monkeypatch.delenv("TMFWM_DEBUG_LIST_CAP")
    _, lap, lst = _single(dev, b, route)
    _check_outputs(out, b, dev, route, order=order)
    assert st == {"lapack_blocks": lap, "list_pass_blocks": lst}, (st, lap, lst)


@pytest.mark.parametrize("b", (4, 16))
def test_many_small_frames(dev, b):
    """70 frames between b x b and 3b x 2b (fewer block rows than list-pass shards per frame), with
    zero-area and no-block frames in between: the frame lookup in the wave, block and shard prefixes.
    The yardstick is the single-size path on each frame alone (the oracle holds it on the frames above)."""
    from thatsmyface_amd import batch

    rng = np.random.default_rng(1500 + b)
    covers, tiles = [], []
    photo = _cover("photo", 6 * b, 4 * b, b)
    for i in range(70):
        H, W = int(rng.integers(b, 3 * b + 1)), int(rng.integers(b, 2 * b + 1))
        if i % 9 == 4:
            H, W = (0, 5) if i % 2 else (b - 1, 2 * b)
        kind = ("photo", "sparks", "photo", "black")[i % 4]
        c = _cover(kind, H, W, b)
        if kind == "photo" and H:  # another crop per frame
            c = np.ascontiguousarray(photo[i % (3 * b):][:H, i % (2 * b):][:, :W])
        covers.append(c)
        tiles.append(_tile(H // b, W // b))
    fr, tt = _dev(covers, dev), _dev(tiles, dev)
    assert all(c.shape[:2] == t.shape[:2] for c, t in zip(covers, fr))
    for route in RANK1:
        lap = lst = 0
        souts = []
        for f, t in zip(fr, tt):
            s1 = {}
            souts.append(batch.embed_batch(f[None], t, b, ALPHA, stats=s1, route=route)[0] if f.numel() else f)
            lap += s1.get("lapack_blocks", 0)
            lst += s1.get("list_pass_blocks", 0)
        st = {}
        out = batch.embed_ragged_rank1(fr, tt, b, ALPHA, stats=st, route=route)
        assert st == {"lapack_blocks": lap, "list_pass_blocks": lst}, (route, st, lap, lst)
        assert (lst if route == "rank1" else lap) > 0
        for i, (o, s) in enumerate(zip(out, souts)):
            assert torch.equal(o, s), (b, route, i)


def _desc(kind, rows):
    arr = (kind * len(rows))()
    for i, r in enumerate(rows):
        arr[i] = kind(*r)
    return arr


@pytest.mark.parametrize("b", (6, 8))
def test_host_memory_through_the_c_entry(dev, b):
    """numpy buffers with canary bytes around every output, the inputs one byte off a 4-byte
    boundary (the byte path), W % 4 != 0: the plain entry on rank1_reference, the key entry on rank1."""
    from thatsmyface_amd import _lib, batch

    L = _lib.load()
    covers, tiles, _, _ = _case(b)
    assert any(c.shape[1] % 4 for c in covers if c.size)
    n = len(covers)
    CAN = 32
    ins, outs, keys = [], [], []
    for c, t in zip(covers, tiles):
        buf = np.zeros(c.size + 8, np.uint8)
        off = 1 + (-buf.ctypes.data) % 4  # one byte past a 4-byte boundary
        buf[off:off + c.size] = c.reshape(-1)
        ins.append((buf, off))
        outs.append(np.full(c.size + 2 * CAN, 0xC3, np.uint8))
        keys.append(np.full(t.size + 2 * CAN // 4, -77.0, np.float32))
    iptr = [buf.ctypes.data + off for buf, off in ins]
    assert all(p % 4 == 1 for p in iptr)
    fr = _dev(covers, dev)
    for route, with_key in (("rank1_reference", False), ("rank1", True)):
        for o in outs:
            o[:] = 0xC3
        _, lap, lst = _single(dev, b, route)
        cnt = ctypes.c_int64(-1)
        if with_key:
            rows = [(iptr[i], outs[i].ctypes.data + CAN, tiles[i].ctypes.data if tiles[i].size else None,
                     keys[i].ctypes.data + CAN if tiles[i].size else None, covers[i].shape[0], covers[i].shape[1]) for i in range(n)]
            d = _desc(_lib.EmbedKeyFrame, rows)
            _lib.check(L.tmfwm_embed_key_ragged_rank1(ctypes.addressof(d), n, b, ALPHA, _lib.MEM_HOST, None, _lib.route_code(route),
                                                      ctypes.addressof(cnt)), "embed_key_ragged_rank1")
            listed = L.tmfwm_last_list_pass_blocks()
            sm = {}
            kref = batch.sigma1_map_ragged([f for f in fr if f.numel()], b, stats=sm)
            assert cnt.value == lap + sm["lapack_blocks"] and listed == lst + sm["list_pass_blocks"], (cnt.value, listed, lap, lst, sm)
            kref = iter(kref)
            for i in range(n):
                if covers[i].size == 0:
                    continue
                want = next(kref).cpu().numpy()
                got = keys[i][CAN // 4:CAN // 4 + tiles[i].size].reshape(tiles[i].shape)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (b, i)
                assert (keys[i][:CAN // 4] == -77.0).all() and (keys[i][CAN // 4 + tiles[i].size:] == -77.0).all(), (b, i)
        else:
            rows = [(iptr[i], outs[i].ctypes.data + CAN, tiles[i].ctypes.data if tiles[i].size else None, covers[i].shape[0],
                     covers[i].shape[1]) for i in range(n)]
            d = _desc(_lib.EmbedFrame, rows)
            _lib.check(L.tmfwm_embed_ragged_rank1(ctypes.addressof(d), n, b, ALPHA, _lib.MEM_HOST, None, _lib.route_code(route),
                                                  ctypes.addressof(cnt)), "embed_ragged_rank1")
            assert cnt.value == lap and L.tmfwm_last_list_pass_blocks() == lst
        _check_outputs([o[CAN:len(o) - CAN].reshape(c.shape) for o, c in zip(outs, covers)], b, dev, route)
        for i, o in enumerate(outs):
            assert (o[:CAN] == 0xC3).all() and (o[len(o) - CAN:] == 0xC3).all(), (b, route, i)
        for (buf, off), c in zip(ins, covers):
            assert np.array_equal(buf[off:off + c.size], c.reshape(-1)) and not buf[:off].any() and not buf[off + c.size:].any()


@pytest.mark.parametrize("route", RANK1)
def test_asynchronous_device_call(dev, route):
    """No stats (nothing synchronises), a stream of the caller's, into the caller's prefilled tensors."""
    from thatsmyface_amd import batch

    b = 10
    covers, tiles, _, _ = _case(b)
    fr, tt = _dev(covers, dev), _dev(tiles, dev)
    given = [torch.full_like(f, 0x5A) for f in fr]
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        got = batch.embed_ragged_rank1(fr, tt, b, ALPHA, out=given, stream=stream, route=route)
    stream.synchronize()
    assert all(g is o for g, o in zip(got, given))
    _check_outputs(got, b, dev, route)


@pytest.mark.parametrize("route", RANK1)
@pytest.mark.parametrize("b", ALL_B)
def test_enrolment(dev, b, route):
    """embed_with_key_ragged_rank1: the embed's pixels, the map's key bits, the counts of both."""
    from thatsmyface_amd import batch

    covers, tiles, _, _ = _case(b)
    fr, tt = _dev(covers, dev), _dev(tiles, dev)
    st, sm = {}, {}
    out, keys = batch.embed_with_key_ragged_rank1(fr, tt, b, ALPHA, stats=st, route=route)
    _check_outputs(out, b, dev, route)
    kref = batch.sigma1_map_ragged(fr, b, stats=sm)
    _, lap, lst = _single(dev, b, route)
    assert len(keys) == len(kref) == len(fr)
    for i, (k, r) in enumerate(zip(keys, kref)):
        assert k.dtype == torch.float32 and k.shape == r.shape == tiles[i].shape
        assert torch.equal(k.view(torch.int32), r.view(torch.int32)), (b, route, i)
    assert st == {"lapack_blocks": lap + sm["lapack_blocks"], "list_pass_blocks": lst + sm["list_pass_blocks"]}, (st, sm, lap, lst)


@pytest.mark.parametrize("route", ("hybrid", "reference"))
@pytest.mark.parametrize("b", (8, 12))
def test_sibling_routes(dev, b, route):
    """The other two routes through the new functions are embed_ragged / embed_with_key_ragged."""
    from thatsmyface_amd import batch

    covers, tiles, _, _ = _case(b)
    fr, tt = _dev(covers, dev), _dev(tiles, dev)
    s0, s1, s2, s3 = {}, {}, {}, {}
    want = batch.embed_ragged(fr, tt, b, ALPHA, stats=s0, route=route)
    got = batch.embed_ragged_rank1(fr, tt, b, ALPHA, stats=s1, route=route)
    wout, wkeys = batch.embed_with_key_ragged(fr, tt, b, ALPHA, stats=s2, route=route)
    gout, gkeys = batch.embed_with_key_ragged_rank1(fr, tt, b, ALPHA, stats=s3, route=route)
    assert s0 == s1 and s2 == s3 and s0["lapack_blocks"] > 0, (s0, s1, s2, s3)
    for i in range(len(fr)):
        assert torch.equal(got[i], want[i]) and torch.equal(gout[i], wout[i]) and torch.equal(got[i], gout[i]), (b, route, i)
        assert torch.equal(gkeys[i].view(torch.int32), wkeys[i].view(torch.int32)), (b, route, i)


@pytest.mark.parametrize("route", ("rank1_reference", "rank1"))
def test_pipeline(dev, route):
    """embed_images over six small images of mixed sizes in groups of four on a rank-1 route: the
    pixels, PNG bytes and keys of the per-image path; extract_images with the same settings: the
    tiles of extract_watermark_keyed."""
    from PIL import Image

    from thatsmyface_amd import pipeline
    from thatsmyface_amd import watermarking as W

    b = 8
    covers, _, _, _ = _case(b)
    picks = [0, 1, 2, 5, 0, 6]
    imgs, wms = [], []
    for k, i in enumerate(picks):
        buf = io.BytesIO()
        Image.fromarray(covers[i]).save(buf, format="PNG")
        imgs.append(buf.getvalue() if k % 2 else Image.fromarray(covers[i]))
        wms.append(Image.fromarray(((O.synth_bytes(0x5EED0002, 20 + k, 1, 29 * 29) & 1) * 255).astype(np.uint8).reshape(29, 29), "L"))
    settings = {"block_size": b, "alpha": ALPHA, "svd_route": route}
    one = pipeline.embed_images(imgs, wms, True, settings, batch_images=None, return_keys=True)
    grp = pipeline.embed_images(imgs, wms, True, settings, batch_images=4, return_keys=True)
    plain = pipeline.embed_images(imgs, wms, True, settings, batch_images=4)
    assert len(one) == len(grp) == len(plain) == 6
    for i, (a, g, p) in enumerate(zip(one, grp, plain)):
        assert np.array_equal(a.pixels, g.pixels) and np.array_equal(a.pixels, p.pixels), (route, i)
        assert a.png == g.png == p.png, (route, i)
        assert a.key.dtype == g.key.dtype == np.float32 and np.array_equal(a.key.view(np.uint32), g.key.view(np.uint32)), (route, i)
        assert p.key is None
    got = list(pipeline.extract_images([g.png if i % 2 else g.image() for i, g in enumerate(grp)], [g.key for g in grp], settings,
                                       batch_images=4))
    for i, (g, e) in enumerate(zip(got, grp)):
        want = W.extract_watermark_keyed(e.image(), e.key, settings)
        assert g.size == want.size and np.array_equal(np.asarray(g), np.asarray(want)), (route, i)
