"""The rank-1 pre-pass's keep / refuse decisions on the GPU against its bound.

embed_rank1_kernel<b> (thatsmyface_amd/csrc/tmfwm_rank1.hip) keeps a block's bytes only with a
proof (its gate and eps_Y) and hands every other block on; the routes count the blocks handed on:
`lapack_blocks` on rank1_reference, `list_pass_blocks` on rank1.  tests/rank1_classes.py sorts a
pool of blocks on the CPU, with the f64 restatement of the same bound, into blocks the kernel must
refuse (undecided even with eps_Y 2 % smaller), blocks it must keep (decided even with eps_Y 2 %
larger and the gate twice as tight) and a thin unclassified band; each class re-tiled into a frame
of its own turns the two counts into the kernel's decisions, class by class.  A must-refuse block
that is kept is a soundness bug of the kernel (an eps_Y too small: the route's guarantee is gone
though nearly every byte still agrees); a must-accept block that is refused is a throughput bug
(an eps_Y too large, a gate that does not open).  tests/test_rank1_bound.py checks on the CPU that
the classes are what this file takes them to be.

Set TMFWM_RANK1_DECISIONS_OUT to a file name to get every frame's counts as JSON
(profiles/rank1_decisions/results.json is such a run)."""
import json
import os

import numpy as np
import pytest

import rank1_classes as RC

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

WIDTHS = (64, 35)  # blocks per frame row: whole strips at every size, and a partial last strip (lanes without a block)
_RESULTS: dict = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from thatsmyface_amd import _lib

    assert _lib.device_count() > 0
    yield torch.device("cuda", 0)
    out = os.environ.get("TMFWM_RANK1_DECISIONS_OUT")
    if out and _RESULTS:
        with open(out, "w") as f:
            json.dump({"refuse_scale": RC.REFUSE_SCALE, "accept_scale": RC.ACCEPT_SCALE, "sentinel_scale": RC.SENTINEL_SCALE,
                       "mirror_scale": RC.MIRROR_SCALE, "accept_scale_widened": None,
                       "counts": {"rank1": "list_pass_blocks", "rank1_reference": "lapack_blocks"}, "sizes": _RESULTS},
                      f, indent=1, sort_keys=True)


def _record(b, key, value):
    _RESULTS.setdefault(str(b), {})[key] = value


def _counts(dev, frame, tile, b, alpha):
    """Blocks the pre-pass left undecided in this frame, per route; every byte the reference
    route's (np.linalg.svd's arithmetic on every block) and the two rank-1 routes' outputs equal."""
    from thatsmyface_amd import batch

    fr, tt = torch.from_numpy(frame[None]).to(dev), torch.from_numpy(tile).to(dev)
    ref = batch.embed_batch(fr, tt, b, alpha, route="reference")
    s1, s2 = {}, {}
    o1 = batch.embed_batch(fr, tt, b, alpha, route="rank1", stats=s1)
    o2 = batch.embed_batch(fr, tt, b, alpha, route="rank1_reference", stats=s2)
    assert torch.equal(o1, ref), (b, alpha, "rank1", int((o1 != ref).sum()))
    assert torch.equal(o2, ref), (b, alpha, "rank1_reference", int((o2 != ref).sum()))
    assert torch.equal(o1, o2)
    return {"blocks": int(tile.size), "rank1": s1["list_pass_blocks"], "rank1_reference": s2["lapack_blocks"]}


def _class_frames(dev, b, cls, alpha, p=None):
    """The counts of class `cls`'s blocks at this alpha, re-tiled at both widths."""
    p = p or RC.pool(b)
    idx = np.nonzero(p[cls] & (p["alpha"] == alpha))[0] if "alpha" in p else np.nonzero(p[cls])[0]
    out = {"members": int(len(idx))}
    for cols in WIDTHS:
        if len(idx):
            fr, t = RC.retile(p["blocks_rgb"][idx], p["tile"][idx], cols)
            out[f"cols{cols}"] = _counts(dev, fr, t, b, alpha)
    return out


def _sizes(b, alpha, p=None):
    p = p or RC.pool(b)
    m = p["alpha"] == alpha if "alpha" in p else np.ones(len(p["tile"]), bool)
    return {k: int((p[k] & m).sum()) for k in ("refuse", "accept", "unclassified", "sentinel", "mirror")}


def _all_refused(r):
    return all(v["rank1"] == v["blocks"] and v["rank1_reference"] == v["blocks"] for k, v in r.items() if k.startswith("cols"))


def _all_kept(r):
    return all(v["rank1"] == 0 and v["rank1_reference"] == 0 for k, v in r.items() if k.startswith("cols"))


@pytest.mark.parametrize("b", RC.SIZES)
def test_sentinels_are_refused(dev, b):
    """The sharpest frame: the must-refuse blocks that a bound 10 % too small would keep, alone.
    The pre-pass refuses every one of them, at each alpha, on both routes."""
    for alpha in RC.ALPHAS:
        r = _class_frames(dev, b, "sentinel", alpha)
        _record(b, f"classes/a{alpha}", _sizes(b, alpha))
        _record(b, f"sentinel/a{alpha}", r)
        assert r["members"] >= 30 and _all_refused(r), (b, alpha, _sizes(b, alpha), r)


@pytest.mark.parametrize("b", RC.SIZES)
def test_must_refuse_blocks_are_refused(dev, b):
    """Every block of the must-refuse frames goes on to the dgesdd route (rank1_reference) and to
    the list pass (rank1): the pre-pass keeps no block it has no proof for.  Blocks the gate alone
    refuses (no spectral gap) are among them; at alpha 0.1, 1.0 and -0.5."""
    for alpha in RC.ALPHAS:
        r = _class_frames(dev, b, "refuse", alpha)
        _record(b, f"refuse/a{alpha}", r)
        if not _all_refused(r):
            pytest.fail(f"b={b} alpha={alpha}: the pre-pass kept must-refuse blocks (a soundness bug): {r}; classes "
                        f"{_sizes(b, alpha)}; the sentinels' own frame: {_class_frames(dev, b, 'sentinel', alpha)}")


@pytest.mark.parametrize("b", RC.SIZES)
def test_must_accept_blocks_are_kept(dev, b):
    """No block of the must-accept frames is handed on, on either route: the bound is no larger
    than stated and the gate opens (zero blocks and DC-only blocks included)."""
    for alpha in RC.ALPHAS:
        r = _class_frames(dev, b, "accept", alpha)
        _record(b, f"accept/a{alpha}", r)
        if not _all_kept(r):
            pytest.fail(f"b={b} alpha={alpha}: the pre-pass refused must-accept blocks (a throughput bug): {r}; classes "
                        f"{_sizes(b, alpha)}; the mirror sentinels' own frame: {_class_frames(dev, b, 'mirror', alpha)}")


@pytest.mark.parametrize("b", RC.SIZES)
def test_whole_frames_count_within_the_band(dev, b):
    """Camera-like frames as they are, blocks of every class side by side in one wave: the count
    lies between the must-refuse blocks and those plus the unclassified ones."""
    p = RC.pool(b)
    frames = RC.pool_frames(b)
    for pick in ("photo13/noise/a0.1", "photo13/binary/a0.1", "photo13/noise/a1.0", "photo14/binary/a-0.5", "qr/a0.1", "noise/a0.1"):
        i = p["names"].index(pick)
        name, cov, t, alpha = frames[i]
        m = p["frame"] == i
        lo, hi = int((p["refuse"] & m).sum()), int(((p["refuse"] | p["unclassified"]) & m).sum())
        r = _counts(dev, np.ascontiguousarray(cov), np.ascontiguousarray(t), b, alpha)
        _record(b, f"whole/{p['names'][i]}", dict(r, must_refuse=lo, unclassified=hi - lo))
        assert lo <= r["rank1"] <= hi and lo <= r["rank1_reference"] <= hi, (b, p["names"][i], lo, hi, r)
        assert r["rank1"] == r["rank1_reference"], (b, p["names"][i], r)


@pytest.mark.parametrize("b", RC.SIZES)
def test_alpha_zero(dev, b):
    """alpha = 0: c = 0 whatever the tile byte, M_fast = D.  The classifier and the kernel agree
    there too: the whole frame's count within the band, and each class's own frame."""
    name, cov, t, _ = RC.pool_frames(b)[0]
    p = RC.classify(cov, t, b, 0.0)
    lo, hi = int(p["refuse"].sum()), int((p["refuse"] | p["unclassified"]).sum())
    r = _counts(dev, np.ascontiguousarray(cov), np.ascontiguousarray(t), b, 0.0)
    ref, acc = _class_frames(dev, b, "refuse", 0.0, p), _class_frames(dev, b, "accept", 0.0, p)
    _record(b, "alpha0", {"whole": dict(r, must_refuse=lo, unclassified=hi - lo), "refuse": ref, "accept": acc, "classes": _sizes(b, 0.0, p)})
    assert lo <= r["rank1"] <= hi and lo <= r["rank1_reference"] <= hi, (b, lo, hi, r)
    assert ref["members"] + acc["members"] >= 0.98 * len(p["tile"]) and ref["members"] > 0 and acc["members"] > 0, (ref, acc)
    assert _all_refused(ref), (b, _sizes(b, 0.0, p), ref)
    assert _all_kept(acc), (b, _sizes(b, 0.0, p), acc)
