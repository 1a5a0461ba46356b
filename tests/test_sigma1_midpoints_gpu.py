"""The extract path's sigma_1 enclosure at float midpoints, on the GPU.  Each fixture
tests/golden/sigma1_midpoints_b<b>.npz is one 4 x 16 block frame holding blocks whose sigma_1 lies
so close to a midpoint between two floats that no enclosure with the kernel's margins can decide
them (must refuse), blocks a little further out that the list pass has to decide (must keep), and
ordinary blocks (tests/sigma1_helpers.py, tests/test_sigma1_midpoints.py).  So on the hybrid route
the number of blocks sent to the dgesdd route is known exactly: the must-refuse ones and no other.
A trimmed margin decides a must-refuse block; a certificate taken for one image of a pair only, or
a list pass that iterates less, changes the count the other way.  Keys and bytes are LAPACK's
throughout, with keys chosen so that one wrong ulp of sigma_1 changes the byte."""
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
import sigma1_helpers as S  # noqa: E402
from keyed_helpers import bytes_of, key_of  # noqa: E402

BLOCKS = (4, 6, 8, 10, 12, 14, 16)
ROUTES = ("hybrid", "reference", "rank1", "rank1_reference")
ALPHAS = (0.1, 1.0, -0.5)
NBH, NBW = 4, 16


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from thatsmyface_amd import _lib

    assert _lib.device_count() > 0
    return torch.device("cuda", 0)


class _Case:
    """One fixture and what the CPU expects of it, computed once per block size."""

    def __init__(self, b):
        fx = np.load(os.path.join(ROOT, "tests", "golden", f"sigma1_midpoints_b{b}.npz"), allow_pickle=False)
        self.b, self.frame = b, np.ascontiguousarray(fx["frame"])
        self.refuse = np.zeros((NBH, NBW), bool)
        self.refuse[tuple(fx["refuse"].T)] = True
        self.listed = self.refuse.copy()
        self.listed[tuple(fx["keep"].T)] = True
        D = S.frame_blocks(self.frame, b)
        self.sigma = S.sigma1_lapack(D).reshape(NBH, NBW)
        self.key_ref = key_of(self.frame, b)
        assert np.array_equal(self.sigma.astype(np.float32), self.key_ref)
        # blocks an enclosure twice as wide as the model's decides after the strip pass's iterations: the
        # ragged calls, which run no list pass, must keep these off the dgesdd route
        self.strip_keeps = S.enclosure(D, S.strip_iters(b), widen=S.KEEP_WIDEN)[2].reshape(NBH, NBW) & ~self.refuse
        self.keys = {}
        for alpha in ALPHAS:
            key, sharp = S.sharpened_key(self.key_ref, self.sigma, self.listed, alpha, seed=b)
            assert sharp[self.listed].all(), (b, alpha)  # every listed block shows a wrong ulp in its byte
            self.keys[alpha] = key


_cases = {}


@pytest.fixture
def case(request):
    b = request.param
    if b not in _cases:
        _cases[b] = _Case(b)
    return _cases[b]


by_size = pytest.mark.parametrize("case", BLOCKS, indirect=True, ids=[f"b{b}" for b in BLOCKS])


def _bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@by_size
def test_key_map_refuses_exactly_the_must_refuse_blocks(dev, case):
    from thatsmyface_amd import batch

    b, nr = case.b, int(case.refuse.sum())
    fr = torch.from_numpy(case.frame[None]).to(dev)
    st = {}
    key = batch.sigma1_map(fr, b, stats=st)
    print(f"b={b}: must-refuse {nr}, stats {st}")
    assert np.array_equal(_bits(key[0]), _bits(case.key_ref))
    assert st["lapack_blocks"] == nr, (st, nr)  # every must-keep and fill block decided, every must-refuse block refused
    assert st["list_pass_blocks"] >= nr, (st, nr)
    for route in ROUTES[1:]:
        sr = {}
        assert np.array_equal(_bits(batch.sigma1_map(fr, b, stats=sr, route=route)[0]), _bits(case.key_ref)), route
        if route == "reference":
            assert sr == {"lapack_blocks": NBH * NBW, "list_pass_blocks": 0}, sr


@by_size
def test_keyed_bytes_with_sharpened_keys(dev, case):
    from thatsmyface_amd import batch

    b, nr = case.b, int(case.refuse.sum())
    fr = torch.from_numpy(case.frame[None]).to(dev)
    for alpha in ALPHAS:
        key = case.keys[alpha]
        exp = bytes_of(case.key_ref, key, alpha)
        st = {}
        got = batch.extract_keyed(fr, torch.from_numpy(key).to(dev), b, alpha, stats=st)
        assert np.array_equal(got[0].cpu().numpy(), exp), (alpha, np.argwhere(got[0].cpu().numpy() != exp))
        assert st["lapack_blocks"] == nr and st["list_pass_blocks"] >= nr, (alpha, st, nr)
        for route in ROUTES[1:]:
            assert np.array_equal(batch.extract_keyed(fr, torch.from_numpy(key[None].copy()).to(dev), b, alpha, route=route)[0].cpu().numpy(),
                                  exp), (alpha, route)


@by_size
def test_pair_path_counts_either_image(dev, case):
    """The fixture against a black original, the roles swapped, and the fixture against itself
    rolled by 8 block columns: a pair goes to the dgesdd route exactly when either image's block is
    a must-refuse one (the interleaved certificates of b <= 14, the sequential ones of b = 16)."""
    from thatsmyface_amd import batch

    b = case.b
    big = 0.75 * b  # sigma_1 of a noise block is about b / 2: quotients inside (0, 1) against the black frame
    black = np.zeros_like(case.frame)
    rolled = np.ascontiguousarray(np.roll(case.frame, 8 * b, axis=1))
    assert len(np.unique(O.extract_frame(case.frame, black, b, big, route="lapack"))) > 8
    none = np.zeros_like(case.refuse)
    pairs = ((case.frame, black, case.refuse, none), (black, case.frame, none, case.refuse),
             (case.frame, rolled, case.refuse, np.roll(case.refuse, 8, axis=1)))
    for i, (w, o, rw, ro) in enumerate(pairs):
        expect = int((rw | ro).sum())
        assert i < 2 or expect > int(rw.sum())  # the rolled copy adds positions of its own
        wt, ot = torch.from_numpy(w[None]).to(dev), torch.from_numpy(o[None]).to(dev)
        for alpha in (0.1, big, -big):
            ref = O.extract_frame(w, o, b, alpha, route="lapack")
            st = {}
            got = batch.extract_batch(wt, ot, b, alpha, stats=st)
            assert np.array_equal(got[0].cpu().numpy(), ref), (i, alpha)
            assert st["lapack_blocks"] == expect and st["list_pass_blocks"] >= expect, (i, alpha, st, expect)
            assert np.array_equal(batch.extract_batch(wt, ot, b, alpha, route="reference")[0].cpu().numpy(), ref), (i, alpha)


@by_size
def test_ragged_calls(dev, case):
    """The fixture frame and its top 2 x 16 blocks in one call.  The ragged calls run no list pass:
    a block undecided after the strip pass's iterations goes to the dgesdd route, so the count is
    bounded on both sides -- every must-refuse block from below, every block that an enclosure twice
    as wide as the model's decides after the strip pass's iterations from above."""
    from thatsmyface_amd import batch

    b = case.b
    top = np.ascontiguousarray(case.frame[: 2 * b])
    frames = [torch.from_numpy(case.frame).to(dev), torch.from_numpy(top).to(dev)]
    lo = int(case.refuse.sum() + case.refuse[:2].sum())
    hi = 3 * NBH * NBW // 2 - int(case.strip_keeps.sum() + case.strip_keeps[:2].sum())
    sm = {}
    keys = batch.sigma1_map_ragged(frames, b, stats=sm)
    print(f"b={b}: ragged key map {sm}, bounds {lo} .. {hi}")
    assert np.array_equal(_bits(keys[0]), _bits(case.key_ref)) and np.array_equal(_bits(keys[1]), _bits(case.key_ref[:2]))
    assert lo <= sm["lapack_blocks"] <= hi and sm["list_pass_blocks"] == 0, (sm, lo, hi)
    for alpha in ALPHAS:
        key = case.keys[alpha]
        kt = [torch.from_numpy(key).to(dev), torch.from_numpy(np.ascontiguousarray(key[:2])).to(dev)]
        exp = bytes_of(case.key_ref, key, alpha)
        sx = {}
        got = batch.extract_keyed_ragged(frames, kt, b, alpha, stats=sx)
        assert np.array_equal(got[0].cpu().numpy(), exp) and np.array_equal(got[1].cpu().numpy(), exp[:2]), alpha
        assert sx == sm, (alpha, sx, sm)  # the same blocks, whatever the key
    # pairs: against the frame rolled by 8 block columns, and against black
    rolled = np.ascontiguousarray(np.roll(case.frame, 8 * b, axis=1))
    either = case.refuse | np.roll(case.refuse, 8, axis=1)
    both = case.strip_keeps & np.roll(case.strip_keeps, 8, axis=1)
    originals = [torch.from_numpy(rolled).to(dev), torch.from_numpy(np.ascontiguousarray(rolled[: 2 * b])).to(dev)]
    lo, hi = int(either.sum() + either[:2].sum()), 3 * NBH * NBW // 2 - int(both.sum() + both[:2].sum())
    for alpha in (0.1, -0.75 * b):
        sp = {}
        got = batch.extract_ragged(frames, originals, b, alpha, stats=sp)
        assert np.array_equal(got[0].cpu().numpy(), O.extract_frame(case.frame, rolled, b, alpha, route="lapack")), alpha
        assert np.array_equal(got[1].cpu().numpy(), O.extract_frame(top, rolled[: 2 * b], b, alpha, route="lapack")), alpha
        assert lo <= sp["lapack_blocks"] <= hi and sp["list_pass_blocks"] == 0, (alpha, sp, lo, hi)
    blacks = [torch.zeros_like(f) for f in frames]
    sp = {}
    got = batch.extract_ragged(frames, blacks, b, 0.75 * b, stats=sp)
    assert np.array_equal(got[0].cpu().numpy(), O.extract_frame(case.frame, np.zeros_like(case.frame), b, 0.75 * b, route="lapack"))
    assert np.array_equal(got[1].cpu().numpy(), O.extract_frame(top, np.zeros_like(top), b, 0.75 * b, route="lapack"))
    assert sp == sm, (sp, sm)  # a black block is decided at once: the count is the key map's


@pytest.mark.parametrize("case", (8, 16), indirect=True, ids=("b8", "b16"))
def test_dropin(dev, case):
    from thatsmyface_amd import watermarking as W

    b = case.b
    img = Image.fromarray(case.frame, "RGB")
    for route in (None, "hybrid"):
        extra = {"svd_route": route} if route else {}
        key = W.extraction_key(img, dict(block_size=b, alpha=0.1, **extra))
        assert key.dtype == np.float32 and np.array_equal(_bits(key), _bits(case.key_ref)), route
        for alpha in ALPHAS:
            ex = W.extract_watermark_keyed(img, case.keys[alpha], dict(block_size=b, alpha=alpha, **extra))
            assert np.array_equal(np.asarray(ex), bytes_of(case.key_ref, case.keys[alpha], alpha)), (route, alpha)
