"""The Jacobi phases of the b = 8 embed strip kernels on the GPU (svd3's forms,
thatsmyface_amd/csrc/tmfwm_device.h: kSvdFlatFirst64, kSvdNormsOnce, kSvdVOnlyEnd; the kernels'
choice of them is in tmfwm_blocks.h): the first f64 sweep branch-free, where a block that skips a
pair takes the identity beside lanes that rotate it, the column norms formed once per phase and
taken from the Newton try's diagonal of G afterwards, and phase 1's last round rotating V32
alone.  Every form keeps the contract's bits, so whichever of them a build switches on, the
frames below -- full and partial strips, waves that mix rotating and non-rotating blocks, blocks
that need second sweeps and the list pass -- must give the oracle's bytes and counts on the embed,
and the oracle's tile on the extract of the result."""
import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

B = 8
NBH = 8  # frames are 8 rows of blocks high
STRUCTURED = ("zero", "flat", "rows", "diagonal", "permutation", "checker")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from thatsmyface_amd import _lib

    assert _lib.device_count() > 0
    return torch.device("cuda", 0)


def _grey(px):
    return np.repeat(px[:, :, None], 3, axis=2)


def _from_dct(D):
    """The grey bytes closest to the block whose DCT is D (luma in [0, 1]): rounding to bytes leaves
    D's pattern with small entries everywhere else, so some pairs rotate and many do not."""
    px = O.dct2d_blocks(D[None].astype(np.float32), inverse=True)[0]
    return _grey(np.clip(np.rint(px * 255.0), 0, 255).astype(np.uint8))


def _structured_block(kind, rng):
    if kind == "zero":  # D == 0: no sweep at all
        return np.zeros((B, B, 3), np.uint8)
    if kind == "flat":  # DC only: every pair's dot product is 0
        return np.full((B, B, 3), int(rng.integers(1, 256)), np.uint8)
    if kind == "rows":  # every pixel row one grey: one non-zero column of D
        return _grey(np.repeat(rng.integers(0, 256, (B, 1), dtype=np.uint8), B, axis=1))
    if kind == "checker":  # two diagonals of D: several f64 sweeps
        return _grey(((np.add.outer(np.arange(B), np.arange(B)) % 2) * 200 + 20).astype(np.uint8))
    D = np.zeros((B, B))
    D[0, 0] = 4.0
    cols = np.arange(1, B) if kind == "diagonal" else rng.permutation(np.arange(1, B))
    D[np.arange(1, B), cols] = 0.2 * np.linspace(1.0, 0.3, B - 1)
    return _from_dct(D)


def _noise_frame(nbw, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (NBH * B, nbw * B, 3), dtype=np.uint8), rng.integers(0, 256, (NBH, nbw), dtype=np.uint8)


def _mixed_frame(seed):
    """One 32-block strip per block row: noise blocks alternate with structured ones, so every wave
    of the strip pass holds rotating lanes beside blocks that skip most or all of their pairs."""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 256, (NBH * B, 32 * B, 3), dtype=np.uint8)
    for i in range(NBH):
        for j in range(1, 32, 2):
            c[i * B:(i + 1) * B, j * B:(j + 1) * B] = _structured_block(STRUCTURED[(i + j // 2) % len(STRUCTURED)], rng)
    t = rng.integers(0, 256, (NBH, 32), dtype=np.uint8)
    t[0, :4] = np.array([0, 255, 255, 0], np.uint8)
    return c, t


def _sweeps(c):
    """Per block, the oracle's f64 sweep count and whether it took the Newton step."""
    y = O.rgb_to_ycbcr(c)[..., 0]
    h, w = y.shape
    blocks = y.reshape(h // B, B, w // B, B).transpose(0, 2, 1, 3).reshape(-1, B, B)
    sw = O.svd_blocks(O.dct2d_blocks(blocks))[3]
    return sw & 0xFF, sw >> 16


def _oracle(c, t, alpha):
    """The reference bytes, the hybrid twin's dgesdd-route count and the extract of the result; the
    twin must agree with the dgesdd route, or the count comparison below would mean nothing."""
    ost = {}
    ref = O.embed_frame(c, t, B, alpha, route="lapack")
    assert np.array_equal(O.embed_frame(c, t, B, alpha, route="hybrid", stats=ost), ref)
    return ref, ost["fallback_blocks"], O.extract_frame(ref, c, B, alpha, route="lapack")


def _check(dev, c, t, alpha):
    from thatsmyface_amd import batch

    ref, fallback, ext = _oracle(c, t, alpha)
    fr, tt = torch.from_numpy(c[None]).to(dev), torch.from_numpy(t).to(dev)
    st = {}
    out = batch.embed_batch(fr, tt, B, alpha, stats=st)
    got = out[0].cpu().numpy()
    assert np.array_equal(got, ref), (alpha, int((got != ref).sum()))
    assert st["lapack_blocks"] == fallback, (alpha, st, fallback)
    gext = batch.extract_batch(out, fr, B, alpha)[0].cpu().numpy()
    assert np.array_equal(gext, ext), (alpha, int((gext != ext).sum()))
    return st, out


def test_oracle_preconditions():
    """From the oracle alone (no GPU work): the mixed strip holds blocks whose first f64 sweep
    rotates no pair beside blocks that rotate, blocks that need further sweeps, and blocks for the
    dgesdd route; on it the hybrid twin gives the dgesdd route's bytes (_oracle asserts that for
    every frame of the cases below as well)."""
    c, t = _mixed_frame(11)
    s64, newton = _sweeps(c)
    s64, newton = s64.reshape(NBH, 32), newton.reshape(NBH, 32)
    still = (s64 <= 1) & (newton == 0)  # stopped after a first sweep without a rotation (or no sweep)
    assert still[:, 1::2].sum() >= NBH * 16 // 3 and not still[:, 0::2].any(), (still.sum(), still[:, 0::2].sum())
    assert (s64[:, 1::2] >= 2).any()
    for alpha in (0.1, -0.05):
        assert _oracle(c, t, alpha)[1] > 0


@pytest.mark.parametrize("alpha", [0.1, -0.05])
@pytest.mark.parametrize("cover", ["noise", "photo"])
@pytest.mark.parametrize("nbw", [32, 35])
def test_full_and_partial_strip(dev, nbw, cover, alpha):
    """32 blocks are one full strip of the b = 8 strip pass, 35 a full and a partial one."""
    from thatsmyface_amd import batch

    c, t = _noise_frame(nbw, 20 + nbw)
    if cover == "photo":
        c = batch.synth_photo_frames(1, NBH * B, nbw * B, seed=77, device=dev)[0].cpu().numpy()
    _check(dev, c, t, alpha)


@pytest.mark.parametrize("alpha", [0.1, -0.05])
def test_mixed_waves(dev, alpha):
    c, t = _mixed_frame(11)
    st, _ = _check(dev, c, t, alpha)
    assert st["lapack_blocks"] > 0, st


def test_second_sweeps_and_list_pass(dev):
    """A camera-like frame, where most blocks take a second f64 sweep after a refused Newton step
    (its norms are the try's diagonal of G), and a noise frame large enough for the list pass."""
    from thatsmyface_amd import batch

    c = batch.synth_photo_frames(1, 128, 256, seed=78, device=dev)[0].cpu().numpy()
    t = np.random.default_rng(36).integers(0, 256, (16, 32), dtype=np.uint8)
    assert (_sweeps(c)[0] >= 2).sum() > 0
    _check(dev, c, t, 0.1)
    c = np.random.default_rng(31).integers(0, 256, (256, 256, 3), dtype=np.uint8)
    t = np.random.default_rng(35).integers(0, 256, (32, 32), dtype=np.uint8)
    assert (_sweeps(c)[0] >= 2).sum() > 0
    st, _ = _check(dev, c, t, 0.1)
    assert st["list_pass_blocks"] > 0, st


def test_keyed_and_ragged_kernels(dev):
    """The key variants and the ragged kernels share the code: the same bytes as embed_batch, which
    the cases above hold to the oracle, and the key of sigma1_map."""
    from thatsmyface_amd import batch

    pairs = [_noise_frame(32, 52), _noise_frame(35, 55), _mixed_frame(11)]
    frames = [torch.from_numpy(c).to(dev) for c, _ in pairs]
    tiles = [torch.from_numpy(t).to(dev) for _, t in pairs]
    alone = [batch.embed_batch(f[None], t, B, 0.1)[0] for f, t in zip(frames, tiles)]
    keys = [batch.sigma1_map(f[None], B)[0] for f in frames]
    for i, (c, t) in enumerate(pairs):
        assert np.array_equal(alone[i].cpu().numpy(), _oracle(c, t, 0.1)[0]), i
        out, key = batch.embed_with_key(frames[i][None], tiles[i], B, 0.1)
        assert torch.equal(out[0], alone[i]), (i, int((out[0] != alone[i]).sum()))
        assert torch.equal(key[0].view(torch.int32), keys[i].view(torch.int32)), i
    outs = batch.embed_ragged(frames, tiles, B, 0.1)
    kouts, kkeys = batch.embed_with_key_ragged(frames, tiles, B, 0.1)
    for i in range(len(pairs)):
        assert torch.equal(outs[i], alone[i]), (i, int((outs[i] != alone[i]).sum()))
        assert torch.equal(kouts[i], alone[i]), (i, int((kouts[i] != alone[i]).sum()))
        assert torch.equal(kkeys[i].view(torch.int32), keys[i].view(torch.int32)), i
