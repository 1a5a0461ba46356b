"""extract_byte / keyed_byte at the values where the byte changes.  The byte is
(s_w - s_o) / f32(alpha) in f32, clipped, * 255.0 in f64, truncated: it changes at quotients next
to k / 255, which pixels produce about once in 10^5 blocks.  A black block's sigma_1 is exactly 0, so
with a black frame a key entry -d makes the numerator any float d: the sweep puts the 7 floats around
every f32(alpha k / 255), and the edges (+-0, a subnormal, alpha itself, an overflowing quotient,
negative quotients), through extract_keyed, extract_keyed_ragged and the drop-in.  A kernel that
multiplied by 1 / alpha instead of dividing gets 262 of these points wrong."""
import os
import sys

import numpy as np
import pytest
from PIL import Image

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sigma1_helpers as S  # noqa: E402
from keyed_helpers import bytes_of  # noqa: E402

NBH, NBW = 16, 1024


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from thatsmyface_amd import _lib

    assert _lib.device_count() > 0
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def sweep():
    """per alpha: the key (NBH, NBW) of entries -d (the points first, +0 after them) and its bytes"""
    out, sharp = {}, 0
    for alpha in S.BYTE_ALPHAS:
        d = S.byte_edge_points(alpha)
        assert len(d) >= 7 * 255 + 8 and len(d) <= NBH * NBW
        key = np.zeros(NBH * NBW, np.float32)
        key[: len(d)] = -d
        exp = bytes_of(np.zeros_like(key), key, alpha)
        sharp += int((exp[: len(d)] != S.byte_by_reciprocal(d, alpha)).sum())
        # every byte is met, and the edges give what the reference's arithmetic gives
        assert set(exp[: 7 * 255]) == set(range(256))
        out[alpha] = (key.reshape(NBH, NBW), exp.reshape(NBH, NBW))
    assert sharp >= 200, sharp  # the sweep tells a multiply by the reciprocal from the division
    return out


@pytest.mark.parametrize("b", (8, 4))
def test_byte_edges_keyed(dev, sweep, b):
    from thatsmyface_amd import batch

    black = torch.zeros((1, NBH * b, NBW * b, 3), dtype=torch.uint8, device=dev)
    for alpha, (key, exp) in sweep.items():
        st = {}
        got = batch.extract_keyed(black, torch.from_numpy(key).to(dev), b, alpha, stats=st).cpu().numpy()[0]
        bad = np.argwhere(got != exp)
        assert len(bad) == 0, (alpha, len(bad), [(key[tuple(p)], got[tuple(p)], exp[tuple(p)]) for p in bad[:5]])
        assert st["lapack_blocks"] == 0, st  # a black block is decided at once
        # the dgesdd route's store is the same function
        got = batch.extract_keyed(black, torch.from_numpy(key).to(dev), b, alpha, route="reference").cpu().numpy()[0]
        assert np.array_equal(got, exp), alpha


@pytest.mark.parametrize("b", (8, 4))
def test_byte_edges_ragged(dev, sweep, b):
    """Two black frames of two sizes: the whole sweep and its top half."""
    from thatsmyface_amd import batch

    frames = [torch.zeros((NBH * b, NBW * b, 3), dtype=torch.uint8, device=dev), torch.zeros((NBH // 2 * b, NBW * b, 3), dtype=torch.uint8, device=dev)]
    for alpha, (key, exp) in sweep.items():
        keys = [torch.from_numpy(key).to(dev), torch.from_numpy(np.ascontiguousarray(key[: NBH // 2])).to(dev)]
        got = batch.extract_keyed_ragged(frames, keys, b, alpha)
        assert np.array_equal(got[0].cpu().numpy(), exp) and np.array_equal(got[1].cpu().numpy(), exp[: NBH // 2]), alpha


@pytest.mark.parametrize("b", (8, 4))
def test_byte_edges_dropin(dev, sweep, b):
    from thatsmyface_amd import watermarking as W

    black = Image.new("RGB", (NBW * b, NBH * b))
    for alpha, (key, exp) in sweep.items():
        ex = W.extract_watermark_keyed(black, key, {"block_size": b, "alpha": alpha, "svd_route": "hybrid"})
        assert np.array_equal(np.asarray(ex), exp), alpha
