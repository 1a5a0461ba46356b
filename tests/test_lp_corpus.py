"""The dgesdd route on inputs that run every branch of it (tests/lp_corpus.py), on the CPU:
numpy == the oracle's restatement == the device header compiled for the host, the oracle's
hybrid route == its dgesdd route on pattern covers, and the coverage record
(tools/lp_coverage.py, tests/golden/lp_unreached.json).  The GPU run of the same inputs is
tests/test_lp_corpus_gpu.py."""
import json
import os
import sys

import numpy as np
import pytest

import lp_corpus as C
from oracle import oracle as O
from test_lapack_device_code import _p, host  # noqa: F401  (host: the header's host build, a fixture)
from test_oracle_lapack import needs_skylakex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORPORA = {"matrices": C.matrices, "bidiagonals": C.bidiagonals}


def _differing(got, ref, labels):
    """Class labels of the blocks in which any factor bit differs."""
    bad = np.zeros(len(labels), bool)
    for x, y in zip(got, ref):
        bad |= (x.view(np.uint32) != y.view(np.uint32)).reshape(len(labels), -1).any(axis=1)
    return sorted({labels[k] for k in np.flatnonzero(bad)}), int(bad.sum())


def test_corpus_is_deterministic_and_labelled():
    for b in (4, 16):
        for fn in CORPORA.values():
            (D, lab), (D2, lab2) = fn(b, 0), fn(b, 0)
            assert D.dtype == np.float32 and D.shape == (len(lab), b, b) and np.isfinite(D).all()
            assert np.array_equal(D.view(np.uint32), D2.view(np.uint32)) and lab == lab2
            assert not np.array_equal(D, fn(b, 1)[0])
    D, lab = C.matrices(8)
    assert {"neg_leading", "zero_rows", "zero_cols", "upper_triangular", "lower_triangular", "orthogonal", "hadamard_like",
            "graded_spectrum_down", "graded_spectrum_up", "cluster", "mixed_scale_rows", "neg_zero"} <= set(lab)
    assert {f"rank_{r}" for r in range(1, 8)} <= set(lab)
    assert np.signbit(D[np.array(lab) == "neg_zero"]).any() and (np.abs(D[D != 0]).min() < C.F32_TINY) and np.abs(D).max() > 1e30
    img, names = C.pattern_cover(16)
    assert img.shape == (24 * 16 + 3, 24 * 16 + 5, 3) and img.dtype == np.uint8 and set(names.ravel()) == set(C.PATTERNS)
    assert np.array_equal(img, C.pattern_cover(16)[0])
    t = C.pattern_tile(24, 24)
    assert (t == 0).any() and (t == 255).any() and len(np.unique(t)) > 50


@needs_skylakex
@pytest.mark.parametrize("b", C.ALL_B)
@pytest.mark.parametrize("corpus", list(CORPORA))
def test_oracle_equals_numpy(corpus, b):
    """np.linalg.svd of the float32 blocks (the factors the reference consumes) == the oracle."""
    D, lab = CORPORA[corpus](b)
    assert _differing(O.lp_svd_blocks(D), np.linalg.svd(D), lab) == ([], 0)


@pytest.mark.parametrize("reverse", [0, 1])
@pytest.mark.parametrize("b", C.ALL_B)
@pytest.mark.parametrize("corpus", list(CORPORA))
def test_device_header_equals_oracle(host, corpus, b, reverse):  # noqa: F811
    """thatsmyface_amd/csrc/tmfwm_lapack.h compiled for the host, under both lane policies
    (reverse = 1 runs every per-element loop backwards), with vectors and S only."""
    D, lab = CORPORA[corpus](b)
    nb = len(D)
    U, Vt, S = np.empty_like(D), np.empty_like(D), np.empty((nb, b), np.float32)
    assert host.lp_host_svd_blocks(_p(D), nb, b, _p(U), _p(S), _p(Vt), 1, reverse) == 0
    ref = O.lp_svd_blocks(D)
    assert _differing((U, S, Vt), ref, lab) == ([], 0)
    S2 = np.empty((nb, b), np.float32)
    assert host.lp_host_svd_blocks(_p(D), nb, b, None, _p(S2), None, 0, reverse) == 0
    assert _differing((S2,), (ref[1],), lab) == ([], 0)


@pytest.mark.parametrize("b", C.ALL_B)
def test_pattern_cover_hybrid_equals_lapack_route(b):
    """Line art and screenshots: most blocks fail the conditioning test and go to the dgesdd
    fallback; the oracle's hybrid route must give the dgesdd route's bytes."""
    cov, _ = C.pattern_cover(b)
    tile = C.pattern_tile(cov.shape[0] // b, cov.shape[1] // b)
    for alpha in (0.1, 1.0, -0.5):
        st = {}
        ref = O.embed_frame(cov, tile, b, alpha, route="lapack")
        assert np.array_equal(O.embed_frame(cov, tile, b, alpha, route="hybrid", stats=st), ref), (b, alpha)
        assert 0 < st["fallback_blocks"] <= tile.size
        assert np.array_equal(O.extract_frame(ref, cov, b, alpha, route="hybrid"),
                              O.extract_frame(ref, cov, b, alpha, route="lapack")), (b, alpha)


def test_unreached_lines_are_recorded():
    """Every line of oracle/tmfwm_lapack.c that the corpora leave unreached (gcc --coverage -O0,
    gcov -b, in a temporary directory) is listed in tests/golden/lp_unreached.json with the
    reason it cannot be reached for float32 input at even b = 4..16.  The cover stand-in is left
    out here (it reaches nothing the other corpora do not, and a smaller set of inputs can only
    leave more unreached)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import lp_coverage as LC

    if not LC.available():
        pytest.skip("gcc / gcov not available")
    with open(os.path.join(ROOT, "tests", "golden", "lp_unreached.json")) as f:
        known = json.load(f)
    assert all(k["reason"].strip() and "no input found" not in k["reason"].lower() for k in known)
    allowed = {(k["routine"], k["line"]) for k in known}
    res = LC.measure(corpora=("patterns", "matrices", "bidiagonals"))
    left = {(u["routine"], u["line"]) for u in LC.unreached(res)}
    assert left <= allowed, sorted(left - allowed)
