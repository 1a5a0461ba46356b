"""Calls with more than 65535 frames, the limit of a grid's y dimension: the C ABI cuts such a
call into chunks of at most 65535 frames (block ids are relative to the chunk), and the launches
that keep no list -- edge pixels of frames without a full block, synthetic frames -- are sliced by
the launcher.  N = 65537 frames, so 65535 + 2.

The frames repeat K = 256 distinct base frames (frame f is base frame f % K, with tile / key
f % K).  The expectation is the same entry point on the K base frames alone, which the parity
tests check against the oracle; it is repeated over all N frames and compared with torch.equal.
Every count of `stats` must equal the base call's count x (N // K) plus the count of a call on the
first N % K base frames: exact, and only so if every listed id past frame 65535 resolves to its own
frame."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N, K = 65537, 256


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda", 0)


def _u8(seed, shape):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def _tiled(base):
    """base[f % K] for f in 0 .. N-1"""
    return base[torch.arange(N, device=base.device) % K].contiguous()


def _check(call, args, what):
    """call(*[a for every frame], stats) against call on the K base frames, repeated; args are
    per-frame tensors of K entries.  Returns (the N results, the base call's stats)."""
    sn, sk, sr = {}, {}, {}
    out = call(*[_tiled(a) for a in args], sn)
    base = call(*args, sk)
    call(*[a[: N % K].contiguous() for a in args], sr)
    print(what, {"all": sn, "base": sk, "rest": sr})
    assert torch.equal(out, _tiled(base)), what
    for k in sk:
        assert sn[k] == sk[k] * (N // K) + sr[k], (what, k, sn, sk, sr)
    return out, sk


def test_tiny_noise_frames_b4(dev):
    """b = 4, 5 x 9 noise frames: 1 x 2 blocks, a right edge column, a bottom edge row, unaligned
    rows.  embed with a tile per frame on three routes, extract, the key map, keyed extract.
    Extract leaves 0.12 % of noise blocks to its list pass at b = 4 (38 of 32768 measured), so
    most seeds give 512 blocks without one; seed 27's frames hold 2 (extract), 2 (key map) and 1
    (keyed extract), and on the rank-1 route embed's list pass takes 510 of the 512."""
    from thatsmyface_amd import batch

    b, a = 4, 0.1
    frames = torch.from_numpy(_u8(27, (K, 5, 9, 3))).to(dev)
    tiles = torch.from_numpy(_u8(12, (K, 1, 2))).to(dev)
    wm = {}
    for route in ("hybrid", "reference", "rank1"):
        wm[route], se = _check(lambda f, t, st: batch.embed_batch(f, t, b, a, stats=st, route=route), (frames, tiles), "embed " + route)
    assert se["list_pass_blocks"] > 0, se  # the last route's: rank1
    assert torch.equal(wm["reference"], wm["hybrid"]) and torch.equal(wm["rank1"], wm["hybrid"])
    wbase = wm["hybrid"][:K].contiguous()
    _, sx = _check(lambda w, o, st: batch.extract_batch(w, o, b, a, stats=st), (wbase, frames), "extract")
    assert sx["list_pass_blocks"] > 0, sx  # extract's list pass holds blocks of frames past 65535
    key, sm = _check(lambda f, st: batch.sigma1_map(f, b, stats=st), (frames,), "sigma1_map")
    _, sk = _check(lambda w, k, st: batch.extract_keyed(w, k, b, a, stats=st), (wbase, key[:K].contiguous()), "extract_keyed")
    assert sm["list_pass_blocks"] > 0 and sk["list_pass_blocks"] > 0, (sm, sk)


def test_embed_list_pass_b8(dev):
    """b = 8, hybrid route, 8 x 64 crops of a camera-like cover (one block row each, cut as
    test_list_pass_segments_vs_oracle cuts its 64 x 128 crops): embed's list pass (b = 8 defers)
    over more than 65535 frames."""
    import sys

    from thatsmyface_amd import batch

    sys.path.insert(0, str(__import__("pathlib").Path(__file__).resolve().parents[1] / "tools" / "exp"))
    from flag_margin import photo_cover

    H, W = 8, 64
    ph = photo_cover(960, 1280, 7)
    crops = [ph[i * H:(i + 1) * H, j * W:(j + 1) * W] for i in range(120) for j in range(20)][:K]
    frames = torch.from_numpy(np.ascontiguousarray(np.stack(crops))).to(dev)
    tiles = torch.from_numpy(_u8(77, (K, H // 8, W // 8))).to(dev)
    _, st = _check(lambda f, t, s: batch.embed_batch(f, t, 8, 0.1, stats=s), (frames, tiles), "embed b=8")
    assert st["list_pass_blocks"] > 0, st


def test_frames_without_a_block(dev):
    """3 x 3 frames at b = 4 hold no full block: the whole call is one edge pass over all N frames,
    which the launcher slices (frame pointers moved per slice).  The colour round trip of a pixel
    does not depend on its frame, so frame f must equal base frame f % K."""
    from thatsmyface_amd import batch

    frames = torch.from_numpy(_u8(13, (K, 3, 3, 3))).to(dev)
    tiles = torch.empty((K, 0, 0), dtype=torch.uint8, device=dev)
    _check(lambda f, t, st: batch.embed_batch(f, t, 4, 0.1, stats=st), (frames, tiles), "edges only")


def test_synth_frames_past_the_slice(dev):
    from thatsmyface_amd import batch

    every = batch.synth_frames(N, 1, 2, device=dev)
    last = batch.synth_frames(2, 1, 2, frame0=65535, device=dev)
    assert torch.equal(every[65535:], last)
    assert torch.equal(every[:2], batch.synth_frames(2, 1, 2, device=dev))
