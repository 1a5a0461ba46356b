"""The embed kernels' colour tail on the GPU (thatsmyface_amd/csrc/tmfwm_colour_tail.h): the f32
decision and the f64 redo together give the bytes and the dgesdd-route block counts of the exact
tail alone -- against the GPU's reference route, the oracle's dgesdd route and the oracle's hybrid
twin, on covers that steer pixels through both paths.  The decision's soundness over all 2^24
colours is the CPU test tests/test_colour_tail.py."""
import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SIZES = [4, 6, 8, 16]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from thatsmyface_amd import _lib

    assert _lib.device_count() > 0
    return torch.device("cuda", 0)


def _u8(seed, shape):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def _cover(kind, b, dev):
    from thatsmyface_amd import batch

    h, w = (256, 256) if (kind == "noise" and b == 8) else (64, 96)
    if kind == "noise":  # ~1000 wave-level pixel steps at b = 8: both paths at the expected rate
        c = _u8(31, (h, w, 3))
    elif kind == "extremes":  # every channel at or next to a clip
        c = np.array([0, 1, 254, 255], np.uint8)[_u8(32, (h, w, 3)) & 3]
    elif kind == "grey":  # flat blocks (D = 0 off the DC term), point intervals, greys on the byte boundary
        c = np.full((h, w, 3), 128, np.uint8)
    else:  # camera-like: decaying spectra, wide intervals
        c = batch.synth_photo_frames(1, h, w, seed=33, device=dev)[0].cpu().numpy()
    if kind == "photo":  # a binary (QR-like) tile: half of the blocks keep their own bytes
        t = (_u8(34, (h // b, w // b)) & np.uint8(1)) * np.uint8(255)
    else:
        t = _u8(35, (h // b, w // b))
    return np.ascontiguousarray(c), t


def _check(dev, c, t, b, alpha, rank1=False):
    from thatsmyface_amd import batch

    fr, tt = torch.from_numpy(c[None]).to(dev), torch.from_numpy(t).to(dev)
    st, ost = {}, {}
    out = batch.embed_batch(fr, tt, b, alpha, stats=st)[0].cpu().numpy()
    gref = batch.embed_batch(fr, tt, b, alpha, route="reference")[0].cpu().numpy()
    ref = O.embed_frame(c, t, b, alpha, route="lapack")
    assert np.array_equal(O.embed_frame(c, t, b, alpha, route="hybrid", stats=ost), ref)
    assert np.array_equal(out, gref), (b, alpha, int((out != gref).sum()))
    assert np.array_equal(out, ref), (b, alpha, int((out != ref).sum()))
    assert st["lapack_blocks"] == ost["fallback_blocks"], (b, alpha, st, ost)
    if rank1:
        for route in ("rank1", "rank1_reference"):
            o = batch.embed_batch(fr, tt, b, alpha, route=route)[0].cpu().numpy()
            assert np.array_equal(o, ref), (b, route, int((o != ref).sum()))


@pytest.mark.parametrize("b", SIZES)
@pytest.mark.parametrize("kind", ["noise", "extremes", "grey", "photo"])
def test_both_tails_give_the_exact_bytes(dev, kind, b):
    c, t = _cover(kind, b, dev)
    _check(dev, c, t, b, 0.1, rank1=kind in ("noise", "photo") and b in (8, 16))


@pytest.mark.parametrize("b", SIZES)
@pytest.mark.parametrize("alpha", [0.0, 1.0, -5.0])
def test_alpha_edges(dev, alpha, b):
    """alpha = 0 (every block keeps its bytes), 1 and -5 (S'[0] < 0: `neg`; Y far outside [0, 1])."""
    c, t = _cover("noise", b, dev)
    c = c[:64, :96]
    _check(dev, np.ascontiguousarray(c), t[: 64 // b, : 96 // b].copy(), b, alpha)


@pytest.mark.parametrize("b", [6, 8])
def test_unaligned_strided_frame(dev, b):
    """A width that is no multiple of 4 bytes, frames at odd offsets and strides: the byte-granular
    row I/O around the colour tail."""
    from thatsmyface_amd import _lib

    h, w = 64 + b // 2, 72 + b + 1
    raw = _u8(36, (3 * h * w * 3 + 7,))
    stride = h * w * 3 + 1
    src = torch.from_numpy(raw).to(dev)
    tile = torch.from_numpy(_u8(37, (h // b, w // b))).to(dev)
    out = torch.zeros_like(src)
    L = _lib.load()
    _lib.check(L.tmfwm_embed(src.data_ptr() + 1, 2, h, w, stride, tile.data_ptr(), b, 0.1, out.data_ptr() + 1, _lib.MEM_DEVICE,
                             torch.cuda.current_stream().cuda_stream), "embed")
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    for f in range(2):
        fr = raw[1 + f * stride: 1 + f * stride + h * w * 3].reshape(h, w, 3)
        ref = O.embed_frame(fr, tile.cpu().numpy(), b, 0.1, route="lapack")
        assert np.array_equal(o[1 + f * stride: 1 + f * stride + h * w * 3].reshape(h, w, 3), ref), (b, f)
