"""Keyed extraction on the GPU: batch.sigma1_map's keys are the oracle's dgesdd
route's f32 S[0] bit for bit on every route, and batch.extract_keyed(w, key) gives the bytes of
the pair path (batch.extract_batch) and of the oracle -- through the strip pass, the list pass,
the dgesdd route, chunking, shared and per-frame keys, host and device memory, the drop-in."""
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


def _three_covers(H, W, seed):
    from golden.gen_golden import cover
    from lapack_path import photo_cover

    return np.ascontiguousarray(np.stack([cover("noise", H, W, seed), photo_cover(H, W, seed + 1), cover("qr", H, W, seed + 2)]))


def _shapes(b):
    # partial strips (35 is no multiple of 64, 32, 16 or 8 blocks per wave), edge pixels and
    # unaligned rows; then whole strips of dword-aligned rows
    return ((3 * b + 3, 35 * b + 5), (4 * b, 64 * b))


@pytest.mark.parametrize("b", BLOCKS)
def test_key_bits_on_both_routes(dev, b):
    from thatsmyface_amd import batch

    for H, W in _shapes(b):
        host = _three_covers(H, W, 10 * b)
        fr = torch.from_numpy(host).to(dev)
        sh, sr = {}, {}
        kh = batch.sigma1_map(fr, b, stats=sh)
        kr = batch.sigma1_map(fr, b, stats=sr, route="reference")
        assert kh.dtype == torch.float32 and tuple(kh.shape) == (3, H // b, W // b)
        assert sr["lapack_blocks"] == 3 * (H // b) * (W // b) and sr["list_pass_blocks"] == 0, sr
        assert sh["lapack_blocks"] < sr["lapack_blocks"], sh
        assert np.array_equal(_bits(kh), _bits(kr)), (H, W)
        for f in range(3):
            assert np.array_equal(_bits(kh[f]), _bits(key_of(host[f], b))), (H, W, f)
        for route in ROUTES[2:]:
            assert np.array_equal(_bits(batch.sigma1_map(fr, b, route=route)), _bits(kh)), route


@pytest.mark.parametrize("b", BLOCKS)
def test_keyed_equals_pair_path_and_oracle(dev, b):
    """One original with three per-frame tiles (a shared key) and three originals (per-frame
    keys), every route name, alpha 0.1 / 1.0 / -0.5, both shapes."""
    from golden.gen_golden import wmark

    from thatsmyface_amd import batch

    for H, W in _shapes(b):
        nbh, nbw = H // b, W // b
        covers = _three_covers(H, W, 20 * b)
        tiles = np.stack([wmark(k, nbh, nbw, 3 + i) for i, k in enumerate(("noise", "qr", "pattern"))])
        tt = torch.from_numpy(tiles).to(dev)
        for shared in (True, False):
            host = np.ascontiguousarray(np.stack([covers[0]] * 3)) if shared else covers
            fr = torch.from_numpy(host).to(dev)
            key = batch.sigma1_map(fr[:1], b)[0] if shared else batch.sigma1_map(fr, b)
            assert key.dim() == (2 if shared else 3)
            for alpha in ALPHAS:
                w = batch.embed_batch(fr, tt, b, alpha)
                w_h = w.cpu().numpy()
                ref = np.stack([O.extract_frame(w_h[f], host[f], b, alpha, route="lapack") for f in range(3)])
                for route in ROUTES:
                    st = {}
                    got = batch.extract_keyed(w, key, b, alpha, route=route, stats=st)
                    pair = batch.extract_batch(w, fr, b, alpha, route=route)
                    assert torch.equal(got, pair), (H, W, shared, alpha, route)
                    assert np.array_equal(got.cpu().numpy(), ref), (H, W, shared, alpha, route)
                    if route == "reference":
                        assert st["lapack_blocks"] == 3 * nbh * nbw and st["list_pass_blocks"] == 0, st
                # asynchronous (no count), into a caller's buffer
                out = torch.full((3, nbh, nbw), 7, dtype=torch.uint8, device=dev)
                assert batch.extract_keyed(w, key, b, alpha, out=out) is out
                torch.cuda.synchronize()
                assert np.array_equal(out.cpu().numpy(), ref)


@pytest.mark.parametrize("b", BLOCKS)
def test_dgesdd_route_taken_on_the_hybrid_route(dev, b):
    """A "sparks" cover (keyed_helpers.sparks): the enclosure can decide no block of it, so on
    the hybrid route every block goes strip pass -> list pass -> dgesdd route."""
    from golden.gen_golden import wmark

    from thatsmyface_amd import batch

    H, W = _shapes(b)[0]
    nbh, nbw = H // b, W // b
    host = np.stack([sparks(H, W, b, 40 + f) for f in range(3)])
    # a frame whose first 17 block columns are noise, the other 18 sparks
    half = sparks(H, W, b, 50)
    half[:, : 17 * b] = _u8(51, (H, 17 * b, 3))
    tile = torch.from_numpy(wmark("noise", nbh, nbw, 4)).to(dev)
    for frames, expect in ((host, 3 * nbh * nbw), (half[None], nbh * (nbw - 17))):
        frames = np.ascontiguousarray(frames)
        fr = torch.from_numpy(frames).to(dev)
        w = batch.embed_batch(fr, tile, b, 0.1)
        sm, sx = {}, {}
        key = batch.sigma1_map(fr, b, stats=sm)
        got = batch.extract_keyed(w, key, b, 0.1, stats=sx)
        assert sm["lapack_blocks"] == expect and sx["lapack_blocks"] == expect, (sm, sx, expect)
        assert sm["list_pass_blocks"] >= expect and sx["list_pass_blocks"] >= expect, (sm, sx)
        assert torch.equal(got, batch.extract_batch(w, fr, b, 0.1))
        w_h = w.cpu().numpy()
        for f in range(len(frames)):
            assert np.array_equal(_bits(key[f]), _bits(key_of(frames[f], b))), f
            assert np.array_equal(got[f].cpu().numpy(), O.extract_frame(w_h[f], frames[f], b, 0.1, route="lapack")), f


def test_list_pass_segments_hold_several_rows(dev):
    """b = 4 on the frames of test_gpu_parity's test_list_pass_segments_vs_oracle (camera-like
    crops, then noise frames): about 3 % of blocks are undecided after the strip pass and take
    the list pass; 300 frames x 16 block rows > 2048 segments, so segments hold several rows."""
    from lapack_path import photo_cover

    from thatsmyface_amd import batch

    b, H, W = 4, 64, 128
    ph = photo_cover(960, 1280, 7)
    crops = [ph[i * H:(i + 1) * H, j * W:(j + 1) * W] for i in range(15) for j in range(10)]
    host = np.ascontiguousarray(np.stack(crops + [_u8(900 + k, (H, W, 3)) for k in range(150)]))
    assert len(host) * (H // b) > 2048
    src = torch.from_numpy(host).to(dev)
    w = batch.embed_batch(src, torch.from_numpy(_u8(77, (H // b, W // b))).to(dev), b, 0.1)
    sm, sx = {}, {}
    key = batch.sigma1_map(src, b, stats=sm)
    got = batch.extract_keyed(w, key, b, 0.1, stats=sx)
    assert sm["list_pass_blocks"] > 0 and sx["list_pass_blocks"] > 0, (sm, sx)
    assert torch.equal(got, batch.extract_batch(w, src, b, 0.1))
    key_h = key.cpu().numpy()
    for f in range(0, len(host), 7):
        assert np.array_equal(_bits(key_h[f]), _bits(key_of(host[f], b))), f


def test_chunked_calls_equal_unchunked(dev, monkeypatch):
    """TMFWM_DEBUG_LIST_CAP at 1.5 frames' worth of ids: one frame per chunk; each chunk's lists,
    counts, key offset (per-frame and shared) and output offset must be its own."""
    from golden.gen_golden import cover

    from thatsmyface_amd import batch

    b, H, W = 8, 64, 128
    nb = (H // b) * (W // b)
    host = np.ascontiguousarray(np.stack([cover("smooth", H, W, 30), sparks(H, W, b, 31), cover("qr", H, W, 32), sparks(H, W, b, 33)]))
    fr = torch.from_numpy(host).to(dev)
    w = batch.embed_batch(fr, torch.from_numpy(_u8(34, (H // b, W // b))).to(dev), b, 0.1)

    def run():
        sm, sx, ss = {}, {}, {}
        key = batch.sigma1_map(fr, b, stats=sm)
        return (key, batch.extract_keyed(w, key, b, 0.1, stats=sx), batch.extract_keyed(w, key[1], b, 0.1, stats=ss)), (sm, sx, ss)

    t0, s0 = run()
    monkeypatch.setenv("TMFWM_DEBUG_LIST_CAP", str(nb * 3 // 2))
    t1, s1 = run()
    assert s0 == s1 and s0[0]["lapack_blocks"] >= 2 * nb and s0[1]["lapack_blocks"] >= 2 * nb, (s0, s1)
    for x, y in zip(t0, t1):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    assert torch.equal(t1[1], batch.extract_batch(w, fr, b, 0.1))
    assert torch.equal(t1[2], batch.extract_batch(w, fr[1:2].expand(4, -1, -1, -1).contiguous(), b, 0.1))


def test_dropin_keyed_equals_pair_on_golden(dev, golden_alpha):
    """extract_watermark_keyed(img_w, extraction_key(img_o)) == extract_watermark(img_w, img_o) ==
    the reference's own bytes, on one golden fixture per block size."""
    from thatsmyface_amd import watermarking as W

    cases, meta = golden_alpha
    seen = set()
    for name, m in meta["cases"].items():
        if m["block"] in seen:
            continue
        seen.add(m["block"])
        arr = cases[f"{name}/cover"]
        cov = Image.fromarray(arr, "L" if arr.ndim == 2 else ("RGBA" if arr.shape[-1] == 4 else "RGB"))
        settings = {"block_size": m["block"], "alpha": m["alpha"]}
        emb = Image.fromarray(cases[f"{name}/embed"])
        key = W.extraction_key(cov, settings)
        assert key.dtype == np.float32 and key.shape == (emb.size[1] // m["block"], emb.size[0] // m["block"])
        ex = W.extract_watermark_keyed(emb, key, settings)
        assert ex.mode == "L"
        assert np.array_equal(np.asarray(ex), np.asarray(W.extract_watermark(emb, cov, settings))), name
        assert np.array_equal(np.asarray(ex), cases[f"{name}/extract"]), name
        for route in ("hybrid", "reference"):
            s = dict(settings, svd_route=route)
            assert np.array_equal(_bits(W.extraction_key(cov, s)), _bits(key)), (name, route)
            assert np.array_equal(np.asarray(W.extract_watermark_keyed(emb, key, s)), cases[f"{name}/extract"]), (name, route)
    assert seen == set(BLOCKS)


def test_malformed_and_negative_key_entries(dev):
    """Non-finite key entries (a damaged file) give byte 0; a finite entry, -1.0 included, gives
    extract_byte's value; the other blocks are untouched."""
    from thatsmyface_amd import batch

    b, H, W = 8, 40, 72
    fr = torch.from_numpy(_u8(60, (2, H, W, 3))).to(dev)
    w = batch.embed_batch(fr, torch.from_numpy(_u8(61, (H // b, W // b))).to(dev), b, 0.1)
    key = batch.sigma1_map(fr, b)
    kw = batch.sigma1_map(w, b).cpu().numpy()
    bad = key.clone()
    bad[0, 0, 0], bad[0, 1, 2], bad[1, 2, 3], bad[1, 4, 8], bad[0, 3, 3] = float("nan"), float("inf"), float("-inf"), -1.0, 3.0e38
    for route in ("hybrid", "reference"):
        for alpha in (0.1, -0.5):
            got = batch.extract_keyed(w, bad, b, alpha, route=route).cpu().numpy()
            finite = np.nan_to_num(bad.cpu().numpy(), nan=0.0, posinf=0.0, neginf=0.0)
            exp = bytes_of(kw, finite, alpha)
            for at in ((0, 0, 0), (0, 1, 2), (1, 2, 3)):
                exp[at] = 0
            assert np.array_equal(got, exp), (route, alpha)
            assert got[1, 4, 8] == (255 if alpha > 0 else 0) and got[0, 3, 3] == (0 if alpha > 0 else 255)
    # sanity of the expectation itself: with the sound key it is the pair path
    assert np.array_equal(bytes_of(kw, key.cpu().numpy(), 0.1), batch.extract_batch(w, fr, b, 0.1).cpu().numpy())


def test_overlap_host_pointers_and_strides(dev):
    from thatsmyface_amd import _lib, batch

    b, H, W, n = 8, 24, 40, 2
    nbh, nbw = H // b, W // b
    host = _u8(70, (n, H, W, 3))
    buf = torch.zeros(n * H * W * 3 + 64, dtype=torch.uint8, device=dev)
    fr = buf[: n * H * W * 3].view(n, H, W, 3)
    fr.copy_(torch.from_numpy(host))
    key = batch.sigma1_map(fr, b)
    ref = batch.extract_keyed(fr, key, b, 0.1)
    # out overlapping an input is refused
    with pytest.raises(ValueError, match="overlaps"):
        batch.sigma1_map(fr, b, out=buf[16: 16 + n * nbh * nbw * 4].view(torch.float32).view(n, nbh, nbw))
    with pytest.raises(ValueError, match="overlaps"):
        batch.extract_keyed(fr, key, b, 0.1, out=buf[8: 8 + n * nbh * nbw].view(n, nbh, nbw))
    with pytest.raises(ValueError, match="overlaps"):
        batch.extract_keyed(fr, key, b, 0.1, out=key.view(torch.uint8).view(-1)[4: 4 + n * nbh * nbw].view(n, nbh, nbw))
    # a host pointer passed as device memory is refused, not dereferenced
    L = _lib.load()
    hk = np.zeros((n, nbh, nbw), np.float32)
    ht = np.zeros((n, nbh, nbw), np.uint8)
    with torch.cuda.device(dev):
        with pytest.raises(ValueError, match="device"):
            _lib.check(L.tmfwm_sigma1_map(host.ctypes.data, n, H, W, H * W * 3, b, key.data_ptr(), _lib.MEM_DEVICE, None, 0, None), "m")
        with pytest.raises(ValueError, match="device"):
            _lib.check(L.tmfwm_sigma1_map(fr.data_ptr(), n, H, W, H * W * 3, b, hk.ctypes.data, _lib.MEM_DEVICE, None, 0, None), "m")
        with pytest.raises(ValueError, match="device"):
            _lib.check(L.tmfwm_extract_keyed(fr.data_ptr(), n, H, W, H * W * 3, hk.ctypes.data, 0, b, 0.1, ref.data_ptr(),
                                             _lib.MEM_DEVICE, None, 0, None), "x")
        with pytest.raises(ValueError, match="device"):
            _lib.check(L.tmfwm_extract_keyed(fr.data_ptr(), n, H, W, H * W * 3, key.data_ptr(), 0, b, 0.1, ht.ctypes.data,
                                             _lib.MEM_DEVICE, None, 0, None), "x")
        # host memory, with padded per-frame keys (key_stride > one key) and a count
        import ctypes

        cnt = ctypes.c_int64(-1)
        _lib.check(L.tmfwm_sigma1_map(host.ctypes.data, n, H, W, H * W * 3, b, hk.ctypes.data, _lib.MEM_HOST, None, 0,
                                      ctypes.addressof(cnt)), "m")
        assert np.array_equal(_bits(hk), _bits(key)) and cnt.value >= 0
        padded = np.full((n, nbh * nbw + 3), np.nan, np.float32)
        padded[:, : nbh * nbw] = hk.reshape(n, -1)
        _lib.check(L.tmfwm_extract_keyed(host.ctypes.data, n, H, W, H * W * 3, padded.ctypes.data, (nbh * nbw + 3) * 4, b, 0.1,
                                         ht.ctypes.data, _lib.MEM_HOST, None, 0, None), "x")
        assert np.array_equal(ht, ref.cpu().numpy())
        # device memory with the same padded stride
        dp = torch.from_numpy(padded).to(dev)
        out = torch.empty_like(ref)
        _lib.check(L.tmfwm_extract_keyed(fr.data_ptr(), n, H, W, H * W * 3, dp.data_ptr(), (nbh * nbw + 3) * 4, b, 0.1,
                                         out.data_ptr(), _lib.MEM_DEVICE, None, 0, ctypes.addressof(cnt)), "x")
        assert torch.equal(out, ref)
    # python-side key checks
    with pytest.raises(TypeError, match="float32"):
        batch.extract_keyed(fr, key.double(), b, 0.1)
    with pytest.raises(ValueError, match="one block size and one image size"):
        batch.extract_keyed(fr, key[:, :2], b, 0.1)
    with pytest.raises(ValueError, match="one block size and one image size"):
        batch.extract_keyed(fr, batch.sigma1_map(fr, 4), b, 0.1)


def test_nonconvergence_reported(dev, monkeypatch):
    from thatsmyface_amd import batch
    from thatsmyface_amd import watermarking as W

    b, h, w = 8, 64, 96
    rgb = _u8(7, (h, w, 3))
    s = {"block_size": b, "alpha": 0.1}
    fr = torch.from_numpy(rgb[None].copy()).to(dev)
    key = batch.sigma1_map(fr, b, stats={})  # sane without the flag
    key_h = W.extraction_key(Image.fromarray(rgb), s)
    assert np.array_equal(_bits(key[0]), _bits(key_h))
    monkeypatch.setenv("TMFWM_DEBUG_FORCE_NONCONV", "1")
    with pytest.raises(RuntimeError, match="did not converge"):
        batch.sigma1_map(fr, b, stats={})
    with pytest.raises(RuntimeError, match="did not converge"):
        batch.extract_keyed(fr, key, b, 0.1, stats={})
    with pytest.raises(RuntimeError, match="did not converge"):
        W.extraction_key(Image.fromarray(rgb), s)
    with pytest.raises(RuntimeError, match="did not converge"):
        W.extract_watermark_keyed(Image.fromarray(rgb), key_h, s)
    batch.extract_keyed(fr, key, b, 0.1)  # async, no count pointer: not checked
    torch.cuda.synchronize()
