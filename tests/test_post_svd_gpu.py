"""The embed kernels between the SVD and the reconstruction on the GPU (embed_blocks,
thatsmyface_amd/csrc/tmfwm_blocks.h): singular values, gaps, the flag, ranks, E_k, the U / S' / B
interval ends.  A block's lanes share that work per triplet (kSplitPost), and the two special
cases -- a zero block, a triplet whose f32(sigma) is 0 -- are written over the ordinary path's
values under a wave-uniform branch (kColdSpecial).  Frames that put special and ordinary blocks
into one wave must give the bytes and the dgesdd-route block counts of the GPU's reference route,
the oracle's dgesdd route and the oracle's hybrid twin."""
import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SIZES = [4, 6, 8, 10, 16]
KINDS = ("noise", "rows", "columns", "black", "grey")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from thatsmyface_amd import _lib

    assert _lib.device_count() > 0
    return torch.device("cuda", 0)


def _frame(b, nbh, nbw, seed):
    """nbh x nbw blocks; block column j is of kind KINDS[j % 5] (at b = 8, 40 columns are one full
    32-block strip and a partial one: special and ordinary blocks share every wave, and lanes
    without a block run too)."""
    rng = np.random.default_rng(seed)
    c = np.empty((nbh * b, nbw * b, 3), np.uint8)
    for i in range(nbh):
        for j in range(nbw):
            kind = KINDS[j % len(KINDS)]
            if kind == "noise":
                blk = rng.integers(0, 256, (b, b, 3), dtype=np.uint8)
            elif kind == "rows":  # every pixel row one colour, the rows differ
                blk = np.repeat(rng.integers(0, 256, (b, 1, 3), dtype=np.uint8), b, axis=1)
            elif kind == "columns":
                blk = np.repeat(rng.integers(0, 256, (1, b, 3), dtype=np.uint8), b, axis=0)
            elif kind == "black":
                blk = np.zeros((b, b, 3), np.uint8)
            else:
                blk = np.full((b, b, 3), 128, np.uint8)
            c[i * b:(i + 1) * b, j * b:(j + 1) * b] = blk
    t = rng.integers(0, 256, (nbh, nbw), dtype=np.uint8)
    t[0, :10] = np.array([0, 255] * 5, np.uint8)  # both extremes on every kind of block
    return c, t


def _sigmas(c, b):
    """Per block of the frame: D (f32 DCT of the luma) and the Jacobi route's f64 singular values."""
    y = O.rgb_to_ycbcr(c)[..., 0]
    h, w = y.shape
    blocks = y.reshape(h // b, b, w // b, b).transpose(0, 2, 1, 3).reshape(-1, b, b)
    D = O.dct2d_blocks(blocks)
    return D, O.svd_blocks_f64(D)[1]


def _kinds_present(c, b):
    D, S = _sigmas(c, b)
    flagged = np.array([O.svd_flag(s) for s in S])
    off_dc = D.reshape(len(D), -1)[:, 1:]
    flat = ~off_dc.any(axis=1)
    zero = ~D.reshape(len(D), -1).any(axis=1)
    lost = (S.astype(np.float32) == 0).any(axis=1)  # a triplet that does not reach the output
    return {"unflagged_lost": int((~flagged & ~flat & ~zero & lost).sum()), "flagged": int(flagged.sum()), "zero": int(zero.sum())}


def _check(dev, c, t, b, alpha):
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
    return st


@pytest.mark.parametrize("b", SIZES)
def test_frame_holds_the_special_blocks(b):
    """The preconditions of the cases below, from the oracle alone (this one needs no GPU work)."""
    c, _ = _frame(b, 4, 40, 50 + b)
    n = _kinds_present(c, b)
    if b in (6, 8, 16):
        assert n["unflagged_lost"] > 0, n
    assert n["flagged"] > 0 and n["zero"] > 0, n


@pytest.mark.parametrize("alpha", [0.1, 0.0, -5.0])
@pytest.mark.parametrize("b", SIZES)
def test_special_and_ordinary_blocks_in_one_wave(dev, b, alpha):
    c, t = _frame(b, 4, 40, 50 + b)
    _check(dev, c, t, b, alpha)


def test_list_pass_runs_the_post_svd_code(dev):
    """256 x 256 noise at b = 8: 1,024 blocks, ~1 % of them need a second sweep and go through
    embed_kernel<8, true>."""
    c = np.random.default_rng(31).integers(0, 256, (256, 256, 3), dtype=np.uint8)
    t = np.random.default_rng(35).integers(0, 256, (32, 32), dtype=np.uint8)
    st = _check(dev, c, t, 8, 0.1)
    assert st["list_pass_blocks"] > 0, st


def test_ragged_frames_of_the_same_blocks(dev):
    """Two frame sizes in one ragged call at b = 8, each against embed_batch on that frame alone."""
    from thatsmyface_amd import batch

    pairs = [_frame(8, 4, 40, 71), _frame(8, 3, 37, 72)]
    frames = [torch.from_numpy(c).to(dev) for c, _ in pairs]
    tiles = [torch.from_numpy(t).to(dev) for _, t in pairs]
    for (c, _), _t in zip(pairs, tiles):
        n = _kinds_present(c, 8)
        assert n["unflagged_lost"] > 0 and n["flagged"] > 0 and n["zero"] > 0, n
    outs = batch.embed_ragged(frames, tiles, 8, 0.1)
    for i, (fr, tt) in enumerate(zip(frames, tiles)):
        alone = batch.embed_batch(fr[None], tt, 8, 0.1)[0]
        assert torch.equal(outs[i], alone), (i, int((outs[i] != alone).sum()))
        assert np.array_equal(alone.cpu().numpy(), O.embed_frame(pairs[i][0], pairs[i][1], 8, 0.1, route="lapack")), i
