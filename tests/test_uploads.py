"""Extract from uploads that are not the embed output, on the CPU: the oracle against
the reference's recorded tiles (tests/golden/cases_uploads.npz, gen_golden.py --uploads), and the
conditions that keep the GPU run (tests/test_uploads_gpu.py) from passing on trivial output --
the expected bytes of every altered class lie inside (0, 255) at one of the extract alphas, and
the sigma_1 enclosure model (tests/sigma1_helpers.py) says how many blocks of such pairs may
reach the dgesdd route: none on camera-like and noise covers, a bounded number on QR covers,
exactly the sparks blocks where one image of a pair is built never to be decided."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
from PIL import Image

from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sigma1_helpers as S  # noqa: E402
import upload_classes as UC  # noqa: E402
from keyed_helpers import bytes_of  # noqa: E402

BLOCKS = UC.BLOCKS
GOLDEN = os.path.join(ROOT, "tests", "golden")


def load_fixture():
    with open(os.path.join(GOLDEN, "meta_uploads.json")) as f:
        meta = json.load(f)
    return np.load(os.path.join(GOLDEN, "cases_uploads.npz"), allow_pickle=False), meta


def fixture_pair(cases, case):
    """(upload RGB u8, original RGB u8 cropped to the upload) as the reference's extract reads them:
    convert("RGB") of both (watermarking.py:242-243), the original's top-left pixels (:269-272)."""
    up = np.asarray(Image.fromarray(cases[case["upload"]], case["upload_mode"]).convert("RGB"))
    orig = np.asarray(Image.fromarray(cases[case["original"]], case["original_mode"]).convert("RGB"))
    return np.ascontiguousarray(up), np.ascontiguousarray(orig[: up.shape[0], : up.shape[1]])


@pytest.fixture(scope="module")
def fixture():
    return load_fixture()


def test_fixture_file_is_the_recorded_one(fixture):
    cases, meta = fixture
    path = os.path.join(GOLDEN, "cases_uploads.npz")
    with open(path, "rb") as f:
        assert hashlib.sha256(f.read()).hexdigest() == meta["sha256_npz"]
    assert os.path.getsize(path) < 1_000_000
    assert meta["alpha"] == 0.1
    names = set(meta["cases"])
    for b in BLOCKS:
        for extra in ("larger_original", "rgba_upload", "l_original"):
            assert f"b{b}/photo/{extra}" in names
        for ck in ("photo", "qr"):
            for cls in ("jpeg75", "noise3", "other"):  # blur and shift are left out at the largest sizes
                assert f"b{b}/{ck}/{cls}" in names
        big = meta["cases"][f"b{b}/photo/larger_original"]
        up, orig = cases[big["upload"]], cases[big["original"]]
        assert orig.shape == (up.shape[0] + 7, up.shape[1] + 11, 3) and up.shape == (5 * b + 3, 9 * b + 5, 3)
        assert meta["cases"][f"b{b}/photo/rgba_upload"]["upload_mode"] == "RGBA" and meta["cases"][f"b{b}/photo/l_original"]["original_mode"] == "L"
    for name, case in meta["cases"].items():
        assert hashlib.sha256(np.ascontiguousarray(cases[case["extract"]]).tobytes()).hexdigest() == case["sha_extract"], name


@pytest.mark.parametrize("b", BLOCKS)
def test_oracle_extracts_the_references_tiles(fixture, b):
    cases, meta = fixture
    seen = 0
    for name, case in meta["cases"].items():
        if case["block"] != b:
            continue
        up, orig = fixture_pair(cases, case)
        want = cases[case["extract"]]
        assert want.shape == (up.shape[0] // b, up.shape[1] // b) and want.dtype == np.uint8
        for route in ("lapack", "hybrid"):
            assert np.array_equal(O.extract_frame(up, orig, b, meta["alpha"], route=route), want), (name, route)
        seen += 1
    assert seen >= 9


def test_jpegish_is_jpeg_shaped():
    """The codec-free class does what a baseline JPEG does to a picture: quantised 8 x 8 DCT
    coefficients (a second pass at the same quality changes little), stronger loss at the lower
    quality, and errors of a JPEG's size."""
    w = UC.corpus(8, "photo").embed
    err = {}
    for q in UC.JPEGISH_QUALITIES:
        j = UC.jpegish(w, q)
        assert j.shape == w.shape and j.dtype == np.uint8
        err[q] = np.abs(j.astype(int) - w.astype(int)).mean()
        again = UC.jpegish(j, q)
        assert np.abs(again.astype(int) - j.astype(int)).mean() < 0.5 * err[q], q
    hi, lo = UC.JPEGISH_QUALITIES
    assert 0.3 < err[hi] < err[lo] < 6.0, err
    flat = np.full((19, 21, 3), 128, np.uint8)
    assert np.array_equal(UC.jpegish(flat, 60), flat)  # a level that every table divides


@pytest.mark.parametrize("b", BLOCKS)
def test_every_class_is_seeded_and_of_one_size(b):
    cp = UC.corpus(b, "photo")
    again = UC.uploads(cp.embed, cp.cover, 1000 * b + 1)
    assert tuple(again) == cp.names and len(cp.names) == 13
    for i, n in enumerate(cp.names):
        assert np.array_equal(again[n][0], cp.up[i]) and np.array_equal(again[n][1], cp.orig[i]), n
        if n not in ("same",):
            assert not np.array_equal(cp.up[i], cp.orig[i]), n
        if n not in ("same", "swapped"):
            assert not np.array_equal(cp.up[i], cp.embed), n  # every other class alters the embed output
    assert cp.up.shape == (13,) + UC.frame_size(b) + (3,) and UC.frame_size(b) == (6 * b + 3, 70 * b + 5)
    from keyed_helpers import key_of

    assert np.array_equal(UC.key_of(cp.up[0], b).view(np.uint32), key_of(cp.up[0], b).view(np.uint32))  # the thread count changes no bit


@pytest.mark.parametrize("kind", ("photo", "noise"))
@pytest.mark.parametrize("b", BLOCKS)
def test_expected_bytes_are_informative(b, kind):
    """For every class that does not clip by construction, at one of the extract alphas at least a
    quarter of the oracle's bytes lie in 1..254 and there are 32 distinct values."""
    cp = UC.corpus(b, kind)
    assert np.array_equal(cp.expect(0.1), bytes_of(cp.keys_up, cp.keys_orig, 0.1))  # the keys are what extract subtracts
    for i, n in enumerate(cp.names):
        per_alpha = {a: bytes_of(cp.keys_up[i], cp.keys_orig[i], a) for a in UC.extract_alphas(b)}
        shares = {a: (round(UC.interior_share(t), 2), len(np.unique(t))) for a, t in per_alpha.items()}
        print(f"b={b} {kind} {n}: interior share / distinct bytes per alpha {shares}")
        if n in UC.CLIPPING:
            continue
        assert any(UC.informative(t) for t in per_alpha.values()), (n, shares)
    # at alpha 0.1 itself the classes close to the embed output are informative already
    for n in ("jpegish90", "jpegish60", "noise3", "blur", "resize", "drop2bits"):
        assert UC.informative(bytes_of(cp.keys_up[cp.names.index(n)], cp.keys_orig[cp.names.index(n)], 0.1)), n


@pytest.mark.parametrize("kind", ("photo", "noise"))
@pytest.mark.parametrize("b", BLOCKS)
def test_model_leaves_no_block_of_a_photo_or_noise_pair_undecided(b, kind):
    """After the list pass's iterations an enclosure twice as wide as the model's decides every
    block of every upload and original: the hybrid route may send none to the dgesdd route."""
    cp = UC.corpus(b, kind)
    cnt = cp.counts
    print(f"b={b} {kind}: strip-pass model leaves {cnt['strip'].sum(axis=(1, 2)).tolist()} undecided per class")
    assert int(cnt["list"].sum()) == 0 and int(cnt["never"].sum()) == 0


@pytest.mark.parametrize("b", BLOCKS)
def test_model_counts_on_qr_pairs(b):
    """On a binary cover many blocks have 2 rho <= F or converge slowly: the counts are what the
    GPU is held to.  A block that can never be decided is undecided in both models; the two models
    do not nest otherwise (a block 640 to 1280 units from a float midpoint is decided by the strip
    model and left by the widened list model)."""
    cp = UC.corpus(b, "qr")
    cnt = cp.counts
    per = {k: v.sum(axis=(1, 2)).tolist() for k, v in cnt.items()}
    print(f"b={b} qr: {per}")
    assert (cnt["never"] <= cnt["list"]).all() and (cnt["never"] <= cnt["strip"]).all()
    assert max(per["list"]) < cnt["list"][0].size // 2  # the bound leaves room: a call that sent every block to the dgesdd route would exceed it


@pytest.mark.parametrize("b", BLOCKS)
def test_sparks_pairs(b):
    """Every sparks block has F > 0 and 2 sigma_1^2 <= F by LAPACK's own sigma_1, so no vector can
    decide it; the photo part of every arrangement is decided by the widened model; so the dgesdd
    route gets exactly the masked positions.  And the pairs' bytes are informative at one of the
    alphas they run at."""
    H, W = UC.frame_size(b)
    nbh, nbw = H // b, W // b  # 6 x 70, 6 x 71 at b = 4
    for seed in (77 + b, 177 + b):
        D = S.frame_blocks(UC.sparks(H, W, b, seed), b)
        F = np.sum(D.astype(np.float64) ** 2, axis=(1, 2))
        s = S.sigma1_lapack(D)
        assert (F > 0.0).all() and (2.0 * s * s <= F).all()
        assert np.allclose(s, 1.0, atol=1e-5) and np.allclose(F, b, atol=1e-4)
    pairs = UC.sparks_pairs(b)
    assert tuple(pairs) == ("orig_sparks", "up_sparks", "orig_cols", "ell")
    for name, (up, orig, mask) in pairs.items():
        cnt = UC.model_counts([up], [orig], b)
        assert np.array_equal(cnt["list"][0], mask), name  # the model: every photo block decided, no sparks block
        assert np.array_equal(cnt["never"][0], mask), name
        assert mask.shape == (nbh, nbw)
        ko, ku = UC.key_of(orig, b), UC.key_of(up, b)
        shares = {a: round(UC.interior_share(bytes_of(ku, ko, a)), 2) for a in UC.sparks_alphas(b)}
        print(f"b={b} {name}: {int(mask.sum())} sparks positions, interior share per alpha {shares}")
        assert any(UC.informative(bytes_of(ku, ko, a)) for a in UC.sparks_alphas(b)), (name, shares)
    assert int(pairs["orig_cols"][2].sum()) == 6 * (nbw - 17) and int(pairs["ell"][2].sum()) == 6 * (nbw - 17) + 3 * 17
    # the L: the lower-left corner is the upload's alone, the upper right the original's alone
    up, orig, _ = pairs["ell"]
    assert UC.never_decided(up, b)[3:, :17].all() and not UC.never_decided(orig, b)[:, :17].any()
    assert UC.never_decided(orig, b)[:3, 17:].all() and not UC.never_decided(up, b)[:3].any()
