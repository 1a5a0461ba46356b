"""The GPU's dgesdd route on inputs that run every reachable branch of it (tests/lp_corpus.py;
what they reach: tools/lp_coverage.py), bit for bit against the oracle, whose
restatement tests/test_lp_corpus.py pins to np.linalg.svd on the same blocks.

The stage entry points take the general and bidiagonal blocks; embed, extract, the keyed and the
ragged calls take the pattern covers (line art, screenshots), whose blocks reach dbdsqr's
zero-shift sweeps in both directions through the second-pass kernels -- as groups of lanes
(most blocks of a pattern cover go to the dgesdd route) and as whole waves (a noise frame with
a few pattern blocks)."""
import functools

import numpy as np
import pytest

import lp_corpus as C
from keyed_helpers import key_of
from oracle import oracle as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ALPHAS = (0.1, 1.0, -0.5)
# the frames are small (about 600 blocks): a team of a few threads, whatever the machine offers
NT = min(8, O.default_threads())


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from thatsmyface_amd import _lib

    assert _lib.device_count() > 0
    return torch.device("cuda", 0)


def _differing(got, ref, labels):
    """(class labels, count) of the blocks in which any bit differs."""
    bad = np.zeros(len(labels), bool)
    for x, y in zip(got, ref):
        x = x.cpu().numpy() if isinstance(x, torch.Tensor) else x
        bad |= (np.ascontiguousarray(x).view(np.uint32) != np.ascontiguousarray(y).view(np.uint32)).reshape(len(labels), -1).any(axis=1)
    return sorted({labels[k] for k in np.flatnonzero(bad)}), int(bad.sum())


@functools.lru_cache(maxsize=None)
def _blocks(b):
    (Dm, lm), (Db, lb) = C.matrices(b), C.bidiagonals(b)
    return np.concatenate([Dm, Db]), lm + lb


@pytest.mark.parametrize("b", C.ALL_B)
def test_lapack_svd_blocks_corpus(dev, b):
    """batch.lapack_svd_blocks (one wave per block) with and without vectors: U, S, Vt == the oracle's."""
    from thatsmyface_amd import batch

    D, lab = _blocks(b)
    ref = O.lp_svd_blocks(D, nthreads=NT)
    Dd = torch.from_numpy(D).to(dev)
    U, S, Vt = batch.lapack_svd_blocks(Dd)
    torch.cuda.synchronize()
    assert _differing((U, S, Vt), ref, lab) == ([], 0)
    _, S2, _ = batch.lapack_svd_blocks(Dd, want_vectors=False)
    assert _differing((S2,), (ref[1],), lab) == ([], 0)


@pytest.mark.parametrize("b", C.ALL_B)
def test_jacobi_svd_blocks_corpus(dev, b):
    """batch.svd_blocks (the Jacobi route) on the same blocks scaled to the range of pixel DCTs
    (sigma_1 in [2^-8, 2^4]): factors and sweep counts == the oracle's."""
    from thatsmyface_amd import batch

    D, lab = _blocks(b)
    D = C.rescale_sigma1(D)
    U, S, Vt, sw = batch.svd_blocks(torch.from_numpy(D).to(dev))
    Uo, So, Vo, swo = O.svd_blocks(D)
    assert _differing((U, S, Vt), (Uo, So, Vo), lab) == ([], 0)
    assert _differing((sw,), (swo,), lab) == ([], 0)


# ------------------------------------------------------------------------------------------------
# pattern covers through the calls
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pattern_case(b):
    """(cover, tile, {alpha: (embed bytes, extracted tile, fallback blocks of the hybrid route)})
    from the oracle's dgesdd route."""
    cov, _ = C.pattern_cover(b)
    tile = C.pattern_tile(cov.shape[0] // b, cov.shape[1] // b)
    return cov, tile, {a: _oracle(cov, tile, b, a) for a in ALPHAS}


def _oracle(cov, tile, b, alpha):
    st = {}
    ref = O.embed_frame(cov, tile, b, alpha, nthreads=NT, route="lapack")
    assert np.array_equal(O.embed_frame(cov, tile, b, alpha, nthreads=NT, route="hybrid", stats=st), ref)
    return ref, O.extract_frame(ref, cov, b, alpha, nthreads=NT, route="lapack"), st["fallback_blocks"]


def _eq(t, ref):
    return np.array_equal(t.cpu().numpy(), ref)


@pytest.mark.parametrize("b", C.ALL_B)
def test_pattern_cover_embed_extract_every_route(dev, b):
    from thatsmyface_amd import batch

    cov, tile, refs = _pattern_case(b)
    fr, tt = torch.from_numpy(cov[None]).to(dev), torch.from_numpy(tile).to(dev)
    for route in ("reference", "hybrid", "rank1", "rank1_reference"):
        for alpha in ALPHAS if route in ("reference", "hybrid") else ALPHAS[:1]:
            ref, ext, nfb = refs[alpha]
            st = {}
            out = batch.embed_batch(fr, tt, b, alpha, stats=st, route=route)
            assert _eq(out[0], ref), (route, alpha)
            if route == "hybrid":
                assert st["lapack_blocks"] == nfb, (alpha, st, nfb)
            if route == "reference":
                assert st["lapack_blocks"] == tile.size
            assert _eq(batch.extract_batch(out, fr, b, alpha, route=route)[0], ext), (route, alpha)


@pytest.mark.parametrize("b", C.ALL_B)
def test_sparse_pattern_cover_whole_wave_second_pass(dev, b):
    """Few enough listed blocks that the hybrid route's second pass takes a whole wave per block
    (the count does not exceed its grid: a wave per 8 blocks at b <= 8, per 4 above)."""
    from thatsmyface_amd import batch

    cov, _ = C.sparse_pattern_cover(b)
    tile = C.pattern_tile(cov.shape[0] // b, cov.shape[1] // b, seed=1)
    ref, ext, nfb = _oracle(cov, tile, b, 0.1)
    assert 0 < nfb <= tile.size // (8 if b <= 8 else 4)
    fr, tt = torch.from_numpy(cov[None]).to(dev), torch.from_numpy(tile).to(dev)
    st, xs = {}, {}
    out = batch.embed_batch(fr, tt, b, 0.1, stats=st)
    assert _eq(out[0], ref) and st["lapack_blocks"] == nfb, (st, nfb)
    assert _eq(batch.extract_batch(out, fr, b, 0.1, stats=xs)[0], ext)
    assert 0 < xs["lapack_blocks"] <= tile.size // (8 if b <= 8 else 4), xs


@pytest.mark.parametrize("b", C.ALL_B)
def test_pattern_cover_keyed(dev, b):
    from thatsmyface_amd import batch

    cov, tile, refs = _pattern_case(b)
    fr = torch.from_numpy(cov[None]).to(dev)
    key_ref = key_of(cov, b).view(np.uint32)
    for route in ("reference", "hybrid"):
        key = batch.sigma1_map(fr, b, route=route)
        assert np.array_equal(key[0].cpu().numpy().view(np.uint32), key_ref), route
        for alpha in ALPHAS:
            ref, ext, _ = refs[alpha]
            w = torch.from_numpy(ref[None]).to(dev)
            assert _eq(batch.extract_keyed(w, key, b, alpha, route=route)[0], ext), (route, alpha)
            assert _eq(batch.extract_keyed(w, key[0].contiguous(), b, alpha, route=route)[0], ext), (route, alpha)


@pytest.mark.parametrize("b", C.ALL_B)
def test_pattern_cover_ragged(dev, b):
    """Two frames of different sizes cut from the cover (13 x 24 blocks with the edge columns,
    11 x 15 blocks with two edge columns and the edge rows), each with its own tile, in one call."""
    from thatsmyface_amd import batch

    cov, tile, _ = _pattern_case(b)
    covers = [np.ascontiguousarray(cov[: 13 * b]), np.ascontiguousarray(cov[13 * b:, : 15 * b + 2])]
    tiles = [np.ascontiguousarray(tile[:13]), np.ascontiguousarray(tile[13:, :15])]
    assert [c.shape[0] // b for c in covers] == [13, 11] and covers[1].shape[0] % b == 3
    fr = [torch.from_numpy(c).to(dev) for c in covers]
    tt = [torch.from_numpy(t).to(dev) for t in tiles]
    for alpha in ALPHAS:
        refs = [_oracle(c, t, b, alpha) for c, t in zip(covers, tiles)]
        for route in ("hybrid", "reference"):
            st = {}
            outs = batch.embed_ragged(fr, tt, b, alpha, stats=st, route=route)
            for o, (ref, _, _) in zip(outs, refs):
                assert _eq(o, ref), (route, alpha)
            want = sum(r[2] for r in refs) if route == "hybrid" else sum(t.size for t in tiles)
            assert st["lapack_blocks"] == want, (route, alpha, st, want)
            exts = batch.extract_ragged(outs, fr, b, alpha, route=route)
            for e, (_, ext, _) in zip(exts, refs):
                assert _eq(e, ext), (route, alpha)
