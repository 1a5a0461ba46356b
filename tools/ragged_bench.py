#!/usr/bin/env python3
"""Ragged batches against the single-size path on the GPU ("Ragged batches").

Workload A (the app's case): 64 camera-like covers with sizes drawn with a fixed seed from
640 x 480 ... 1920 x 1080, a QR tile per image, b = 8, alpha 0.1, hybrid route, frames resident
on the device.  One embed_ragged + one extract_ragged against the loop of 64 single-frame
embed_batch / extract_batch calls.

Workload B (the cost of the frame table and of going without the list pass): 256 frames of
1920 x 1080 at b = 8 and b = 16, on noise covers and on camera-like covers; embed_ragged against
embed_batch (a tile per frame) on the same frames.

Workload K (ragged keyed extraction): workload A's frames, embedded once, with their
keys resident on the device.  Three comparisons: extract_keyed_ragged against the loop of 64
single-frame extract_keyed calls; extract_keyed_ragged against extract_ragged with the originals
(the pair path; its time is reported as "base"); sigma1_map_ragged against the loop of 64
single-frame sigma1_map calls.

Workload E (enrolment): workload A's frames and tiles.  embed_with_key_ragged against
embed_ragged followed by sigma1_map_ragged (the two-pass way to the same outputs and keys; its
time is reported as "base"), and against embed_ragged alone (what the key costs).

Workload R (the rank-1 routes): workload A's frames and tiles at b = 8 and b = 16.
embed_ragged_rank1 on "rank1" against embed_ragged on "hybrid" (base), on "rank1_reference" against
embed_ragged on "reference" (base), and each of the two against the loop of 64 single-frame
embed_batch calls on the same rank-1 route (base).

Workload S (one alpha per frame): workload A's frames and tiles with 64 distinct
alphas in [0.02, 0.5].  embed_ragged(alpha=list) against the loop of 64 single-frame embed_batch
calls at those alphas (base); extract_keyed_ragged(alpha=list) against its loop (base); and each of
the two against the same call with one alpha (base): what the per-frame form costs.  With
--parent-lib PATH (a libtmfwm.so built from the parent commit, loaded into the same process) also
the uniform embed_ragged and extract_keyed_ragged of this build against the parent's (base).

Both arms of a comparison run alternately in one process, each timing a window of `inner` calls
that ends in a device synchronise.  Every ratio comes with the A/A spread of its own run: the
medians of the even and of the odd rounds of the same arm, as a ratio.  The arms' outputs are
compared byte for byte before anything is timed.

usage: python tools/ragged_bench.py [--workload a|b|k|e|r|s|ab|abk] [--rounds R] [--frames-b N] [--parent-lib PATH]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from thatsmyface_amd import _lib, batch  # noqa: E402

SIZES = [(480, 640), (600, 800), (768, 1024), (720, 1280), (1080, 1920)]  # (H, W)


def window(fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / inner


def compare(name, arms, inner, rounds, extra):
    """arms: {"base": fn, "ragged": fn}; alternating rounds; prints one JSON line."""
    for fn in arms.values():  # warm-up: code objects, pools, allocator
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            t[k].append(window(fn, inner))
    med = {k: statistics.median(v) for k, v in t.items()}
    aa = {k: statistics.median(v[0::2]) / statistics.median(v[1::2]) for k, v in t.items()}
    rec = {"workload": name, **extra, "inner": inner, "rounds": rounds,
           "base_ms": round(1e3 * med["base"], 4), "ragged_ms": round(1e3 * med["ragged"], 4),
           "ragged_over_base": round(med["ragged"] / med["base"], 4),
           "aa_base": round(aa["base"], 4), "aa_ragged": round(aa["ragged"], 4),
           "min_ms": {k: round(1e3 * min(v), 4) for k, v in t.items()}, "max_ms": {k: round(1e3 * max(v), 4) for k, v in t.items()}}
    print(json.dumps(rec), flush=True)
    return rec


def frames_a(dev, b, n):
    """Workload A's covers and tiles: (picks, frames, tiles)."""
    rng = np.random.default_rng(20240)
    picks = [SIZES[int(k)] for k in rng.integers(0, len(SIZES), n)]
    frames = [batch.synth_photo_frames(1, h, w, seed=7000 + i, device=dev)[0].contiguous() for i, (h, w) in enumerate(picks)]
    tiles = [batch.synth_qr_tile(h // b, w // b, seed=8000 + i, device=dev) for i, (h, w) in enumerate(picks)]
    return picks, frames, tiles


def workload_a(rounds, dev):
    b, alpha, n = 8, 0.1, 64
    picks, frames, tiles = frames_a(dev, b, n)
    frames1 = [f[None] for f in frames]
    state = {}

    def loop():
        outs = [batch.embed_batch(f, t, b, alpha) for f, t in zip(frames1, tiles)]
        state["loop"] = (outs, [batch.extract_batch(o, f, b, alpha) for o, f in zip(outs, frames1)])

    def ragged():
        outs = batch.embed_ragged(frames, tiles, b, alpha)
        state["ragged"] = (outs, batch.extract_ragged(outs, frames, b, alpha))

    loop()
    ragged()
    torch.cuda.synchronize()
    for i in range(n):
        assert torch.equal(state["loop"][0][i][0], state["ragged"][0][i]), ("embed differs", i)
        assert torch.equal(state["loop"][1][i][0], state["ragged"][1][i]), ("extract differs", i)
    mp = sum(h * w for h, w in picks) / 1e6
    sizes = {f"{w}x{h}": picks.count((h, w)) for h, w in SIZES}
    return compare("A", {"base": loop, "ragged": ragged}, 10, rounds,
                   {"what": "64 images embed+extract: ragged vs loop of single-frame calls", "block": b, "megapixels": round(mp, 1),
                    "sizes": sizes, "outputs_equal": True})


def workload_k(rounds, dev):
    b, alpha, n = 8, 0.1, 64
    picks, frames, tiles = frames_a(dev, b, n)
    wm = batch.embed_ragged(frames, tiles, b, alpha)
    frames1, wm1 = [f[None] for f in frames], [w[None] for w in wm]
    keys = batch.sigma1_map_ragged(frames, b)
    state = {}
    arms = {
        "keyed_loop": lambda: state.__setitem__("keyed_loop", [batch.extract_keyed(w, k, b, alpha) for w, k in zip(wm1, keys)]),
        "keyed_ragged": lambda: state.__setitem__("keyed_ragged", batch.extract_keyed_ragged(wm, keys, b, alpha)),
        "pair_ragged": lambda: state.__setitem__("pair_ragged", batch.extract_ragged(wm, frames, b, alpha)),
        "map_loop": lambda: state.__setitem__("map_loop", [batch.sigma1_map(f, b) for f in frames1]),
        "map_ragged": lambda: state.__setitem__("map_ragged", batch.sigma1_map_ragged(frames, b)),
    }
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    for i in range(n):
        assert torch.equal(state["keyed_loop"][i][0], state["keyed_ragged"][i]), ("keyed extract differs from the loop", i)
        assert torch.equal(state["pair_ragged"][i], state["keyed_ragged"][i]), ("keyed extract differs from the pair path", i)
        assert torch.equal(state["map_loop"][i][0].view(torch.int32), state["map_ragged"][i].view(torch.int32)), ("key differs", i)
    sm, sx = {}, {}
    batch.sigma1_map_ragged(frames, b, stats=sm)
    batch.extract_keyed_ragged(wm, keys, b, alpha, stats=sx)
    extra = {"block": b, "megapixels": round(sum(h * w for h, w in picks) / 1e6, 1), "outputs_equal": True,
             "lapack_blocks_map": sm["lapack_blocks"], "lapack_blocks_extract": sx["lapack_blocks"]}
    return [compare("K1", {"base": arms["keyed_loop"], "ragged": arms["keyed_ragged"]}, 10, rounds,
                    {"what": "64 images keyed extract: extract_keyed_ragged vs loop of single-frame extract_keyed", **extra}),
            compare("K2", {"base": arms["pair_ragged"], "ragged": arms["keyed_ragged"]}, 10, rounds,
                    {"what": "64 images extract: extract_keyed_ragged vs extract_ragged with the originals (base)", **extra}),
            compare("K3", {"base": arms["map_loop"], "ragged": arms["map_ragged"]}, 10, rounds,
                    {"what": "64 images key maps: sigma1_map_ragged vs loop of single-frame sigma1_map", **extra})]


def workload_e(rounds, dev):
    b, alpha, n = 8, 0.1, 64
    picks, frames, tiles = frames_a(dev, b, n)
    state = {}

    def two_pass():
        state["two_pass"] = (batch.embed_ragged(frames, tiles, b, alpha), batch.sigma1_map_ragged(frames, b))

    arms = {
        "two_pass": two_pass,
        "with_key": lambda: state.__setitem__("with_key", batch.embed_with_key_ragged(frames, tiles, b, alpha)),
        "embed": lambda: state.__setitem__("embed", batch.embed_ragged(frames, tiles, b, alpha)),
    }
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    for i in range(n):
        assert torch.equal(state["two_pass"][0][i], state["with_key"][0][i]), ("embed differs", i)
        assert torch.equal(state["two_pass"][1][i].view(torch.int32), state["with_key"][1][i].view(torch.int32)), ("key differs", i)
    se, sm, sk = {}, {}, {}
    batch.embed_ragged(frames, tiles, b, alpha, stats=se)
    batch.sigma1_map_ragged(frames, b, stats=sm)
    batch.embed_with_key_ragged(frames, tiles, b, alpha, stats=sk)
    extra = {"block": b, "megapixels": round(sum(h * w for h, w in picks) / 1e6, 1), "outputs_equal": True,
             "lapack_blocks_embed": se["lapack_blocks"], "lapack_blocks_map": sm["lapack_blocks"], "lapack_blocks_with_key": sk["lapack_blocks"]}
    return [compare("E1", {"base": arms["two_pass"], "ragged": arms["with_key"]}, 10, rounds,
                    {"what": "64 images enrolment: embed_with_key_ragged vs embed_ragged + sigma1_map_ragged (base)", **extra}),
            compare("E2", {"base": arms["embed"], "ragged": arms["with_key"]}, 10, rounds,
                    {"what": "64 images enrolment: embed_with_key_ragged vs embed_ragged alone (base)", **extra})]


def workload_r(rounds, dev):
    alpha, n = 0.1, 64
    out = []
    for b in (8, 16):
        picks, frames, tiles = frames_a(dev, b, n)
        frames1 = [f[None] for f in frames]
        state = {}

        def loop(route):
            return lambda: state.__setitem__("loop_" + route, [batch.embed_batch(f, t, b, alpha, route=route) for f, t in zip(frames1, tiles)])

        arms = {
            "hybrid": lambda: state.__setitem__("hybrid", batch.embed_ragged(frames, tiles, b, alpha, route="hybrid")),
            "reference": lambda: state.__setitem__("reference", batch.embed_ragged(frames, tiles, b, alpha, route="reference")),
            "rank1": lambda: state.__setitem__("rank1", batch.embed_ragged_rank1(frames, tiles, b, alpha, route="rank1")),
            "rank1_reference": lambda: state.__setitem__("rank1_reference",
                                                         batch.embed_ragged_rank1(frames, tiles, b, alpha, route="rank1_reference")),
            "loop_rank1": loop("rank1"),
            "loop_rank1_reference": loop("rank1_reference"),
        }
        for fn in arms.values():
            fn()
        torch.cuda.synchronize()
        for i in range(n):  # every route gives the reference's bytes
            for k in ("hybrid", "rank1", "rank1_reference"):
                assert torch.equal(state[k][i], state["reference"][i]), (k, "differs from the reference route", b, i)
            for k in ("loop_rank1", "loop_rank1_reference"):
                assert torch.equal(state[k][i][0], state["reference"][i]), (k, "differs from the reference route", b, i)
        st = {}
        for route in ("rank1", "rank1_reference"):
            s1 = {}
            batch.embed_ragged_rank1(frames, tiles, b, alpha, stats=s1, route=route)
            st[route] = s1
        blocks = sum((h // b) * (w // b) for h, w in picks)
        extra = {"block": b, "megapixels": round(sum(h * w for h, w in picks) / 1e6, 1), "blocks": blocks, "outputs_equal": True,
                 "stats": st}
        out += [compare("R1", {"base": arms["hybrid"], "ragged": arms["rank1"]}, 10, rounds,
                        {"what": "64 images embed: embed_ragged_rank1 rank1 vs embed_ragged hybrid (base)", **extra}),
                compare("R2", {"base": arms["reference"], "ragged": arms["rank1_reference"]}, 2, rounds,
                        {"what": "64 images embed: embed_ragged_rank1 rank1_reference vs embed_ragged reference (base)", **extra}),
                compare("R3", {"base": arms["loop_rank1"], "ragged": arms["rank1"]}, 10, rounds,
                        {"what": "64 images embed: embed_ragged_rank1 rank1 vs loop of single-frame embed_batch rank1 (base)", **extra}),
                compare("R4", {"base": arms["loop_rank1_reference"], "ragged": arms["rank1_reference"]}, 10, rounds,
                        {"what": "64 images embed: embed_ragged_rank1 rank1_reference vs loop of single-frame embed_batch "
                                 "rank1_reference (base)", **extra})]
        del frames, tiles, frames1, state
        torch.cuda.empty_cache()
    return out


def other_build(path):
    """fn -> fn run on another build of the library (same ABI) in this process (_lib.open_build /
    _lib.using), so both builds are timed in alternating windows of one run."""
    other = _lib.open_build(path)

    def on_other(fn):
        def run():
            with _lib.using(other):
                return fn()

        return run

    return on_other


def workload_s(rounds, dev, parent_lib):
    b, n = 8, 64
    picks, frames, tiles = frames_a(dev, b, n)
    alphas = [float(a) for a in np.linspace(0.02, 0.5, n)]
    assert len(set(alphas)) == n
    frames1 = [f[None] for f in frames]
    wm = batch.embed_ragged(frames, tiles, b, alphas)
    wm1 = [w[None] for w in wm]
    keys = batch.sigma1_map_ragged(frames, b)
    state = {}
    arms = {
        "embed_loop": lambda: state.__setitem__("embed_loop", [batch.embed_batch(f, t, b, a) for f, t, a in zip(frames1, tiles, alphas)]),
        "embed_alphas": lambda: state.__setitem__("embed_alphas", batch.embed_ragged(frames, tiles, b, alphas)),
        "embed_uniform": lambda: state.__setitem__("embed_uniform", batch.embed_ragged(frames, tiles, b, 0.1)),
        "embed_alphas_same": lambda: state.__setitem__("embed_alphas_same", batch.embed_ragged(frames, tiles, b, [0.1] * n)),
        "keyed_loop": lambda: state.__setitem__("keyed_loop", [batch.extract_keyed(w, k, b, a) for w, k, a in zip(wm1, keys, alphas)]),
        "keyed_alphas": lambda: state.__setitem__("keyed_alphas", batch.extract_keyed_ragged(wm, keys, b, alphas)),
        "keyed_uniform": lambda: state.__setitem__("keyed_uniform", batch.extract_keyed_ragged(wm, keys, b, 0.1)),
        "keyed_alphas_same": lambda: state.__setitem__("keyed_alphas_same", batch.extract_keyed_ragged(wm, keys, b, [0.1] * n)),
    }
    if parent_lib:
        on_parent = other_build(parent_lib)
        arms["embed_parent"] = on_parent(lambda: state.__setitem__("embed_parent", batch.embed_ragged(frames, tiles, b, 0.1)))
        arms["keyed_parent"] = on_parent(lambda: state.__setitem__("keyed_parent", batch.extract_keyed_ragged(wm, keys, b, 0.1)))
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    for i in range(n):
        assert torch.equal(state["embed_loop"][i][0], state["embed_alphas"][i]), ("embed differs from the loop", i)
        assert torch.equal(state["embed_loop"][i][0], wm[i]), ("embed differs from the loop", i)
        assert torch.equal(state["keyed_loop"][i][0], state["keyed_alphas"][i]), ("keyed extract differs from the loop", i)
        assert torch.equal(state["embed_uniform"][i], state["embed_alphas_same"][i]), ("the per-frame form differs from the uniform one", i)
        assert torch.equal(state["keyed_uniform"][i], state["keyed_alphas_same"][i]), ("the per-frame form differs from the uniform one", i)
        if parent_lib:
            assert torch.equal(state["embed_uniform"][i], state["embed_parent"][i]), ("embed differs from the parent build", i)
            assert torch.equal(state["keyed_uniform"][i], state["keyed_parent"][i]), ("keyed extract differs from the parent build", i)
    extra = {"block": b, "megapixels": round(sum(h * w for h, w in picks) / 1e6, 1), "alphas": [alphas[0], alphas[-1]], "outputs_equal": True}
    out = [compare("S1", {"base": arms["embed_loop"], "ragged": arms["embed_alphas"]}, 10, rounds,
                   {"what": "64 images, 64 alphas, embed: embed_ragged(alpha=list) vs loop of single-frame embed_batch (base)", **extra}),
           compare("S2", {"base": arms["keyed_loop"], "ragged": arms["keyed_alphas"]}, 10, rounds,
                   {"what": "64 images, 64 alphas, keyed extract: extract_keyed_ragged(alpha=list) vs loop of single-frame extract_keyed "
                            "(base)", **extra}),
           compare("S3", {"base": arms["embed_uniform"], "ragged": arms["embed_alphas"]}, 10, rounds,
                   {"what": "64 images embed: embed_ragged(alpha=list) vs embed_ragged with one alpha (base)", **extra}),
           compare("S4", {"base": arms["keyed_uniform"], "ragged": arms["keyed_alphas"]}, 10, rounds,
                   {"what": "64 images keyed extract: extract_keyed_ragged(alpha=list) vs extract_keyed_ragged with one alpha (base)", **extra})]
    if parent_lib:
        out += [compare("S5", {"base": arms["embed_parent"], "ragged": arms["embed_uniform"]}, 10, rounds,
                        {"what": "64 images embed, one alpha: embed_ragged of this build vs the parent commit's build (base)", **extra}),
                compare("S6", {"base": arms["keyed_parent"], "ragged": arms["keyed_uniform"]}, 10, rounds,
                        {"what": "64 images keyed extract, one alpha: extract_keyed_ragged of this build vs the parent commit's build (base)",
                         **extra})]
    return out


def workload_b(rounds, dev, n):
    out = []
    for cover in ("noise", "photo"):
        h, w = 1080, 1920
        frames = batch.synth_photo_frames(n, h, w, device=dev) if cover == "photo" else batch.synth_frames(n, h, w, device=dev)
        views = [frames[i] for i in range(n)]
        for b in (8, 16):
            tiles = torch.stack([batch.synth_tile(h // b, w // b, seed=9000 + i, device=dev) for i in range(n)])
            tviews = [tiles[i] for i in range(n)]
            dst = torch.empty_like(frames)
            dviews = [dst[i] for i in range(n)]
            ref = batch.embed_batch(frames, tiles, b, 0.1)
            st_b, st_r = {}, {}
            batch.embed_batch(frames, tiles, b, 0.1, out=dst, stats=st_b)
            got = batch.embed_ragged(views, tviews, b, 0.1, out=dviews, stats=st_r)
            torch.cuda.synchronize()
            assert torch.equal(torch.stack(got), ref), ("embed differs", cover, b)
            assert st_b["lapack_blocks"] == st_r["lapack_blocks"], (st_b, st_r)
            del ref, got
            arms = {"base": lambda: batch.embed_batch(frames, tiles, b, 0.1, out=dst),
                    "ragged": lambda: batch.embed_ragged(views, tviews, b, 0.1, out=dviews)}
            out.append(compare("B", arms, 4, rounds,
                               {"what": f"{n} x 1080p embed: ragged vs embed_batch", "cover": cover, "block": b,
                                "lapack_blocks": st_b["lapack_blocks"], "list_pass_blocks_base": st_b["list_pass_blocks"],
                                "outputs_equal": True}))
            del tiles, tviews, dst, dviews
        del frames, views
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="ab", choices=("a", "b", "k", "e", "r", "s", "ab", "abk"))
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--frames-b", type=int, default=256)
    ap.add_argument("--parent-lib", default=None, help="workload s: a libtmfwm.so of the parent commit to time the uniform calls against")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ragged_bench: no GPU (there is no CPU fallback to time)")
    dev = torch.device("cuda", 0)
    print(json.dumps({"device": torch.cuda.get_device_name(0), "rounds": a.rounds}), flush=True)
    if "a" in a.workload:
        workload_a(a.rounds, dev)
    if "b" in a.workload:
        workload_b(a.rounds, dev, a.frames_b)
    if "k" in a.workload:
        workload_k(a.rounds, dev)
    if "e" in a.workload:
        workload_e(a.rounds, dev)
    if "r" in a.workload:
        workload_r(a.rounds, dev)
    if "s" in a.workload:
        workload_s(a.rounds, dev, a.parent_lib)


if __name__ == "__main__":
    main()
