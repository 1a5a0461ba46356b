#!/usr/bin/env python3
"""Tile preparation for a batch of mixed sizes on the GPU ("Ragged tile preparation").

Workload: the 64 seeded size picks of tools/ragged_bench.py's workload A (640 x 480 ... 1920 x 1080),
64 distinct binary 300 x 300 watermarks resident on the device, preserve_ratio on, b = 8.

Arms: (a) 64 prepare_tile calls, the only way without the ragged call; (b) one
prepare_tiles_ragged; (c) five prepare_tiles calls, the watermarks grouped by size on the host
(stacked once, outside the timed region): the best a caller could do before.  End to end:
(a) + embed_ragged against (b) + embed_ragged.  Worst case for the axis deduplication: 64
all-distinct tile sizes without preserve_ratio (128 distinct axes), arms (a) and (b).

The arms' bytes are compared first.  The arms of a comparison run alternately in one process;
every window holds at least `--window` seconds of calls and ends in a device synchronise.  Medians
over the rounds, and per arm the A/A figure: the median of its even rounds over that of its odd
rounds.

usage: python tools/tile_ragged_time.py [--rounds R] [--window SECONDS]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from thatsmyface_amd import batch  # noqa: E402
from tools.ragged_bench import SIZES  # noqa: E402


def window(fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / inner


def compare(name, arms, rounds, seconds, extra):
    """arms: {label: fn}; alternating rounds; prints one JSON line."""
    inner = {}
    for k, fn in arms.items():  # warm-up (code objects, pools, allocator), then the calls a window needs
        for _ in range(3):
            fn()
        inner[k] = max(3, math.ceil(seconds / window(fn, 3)))
    t = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            t[k].append(window(fn, inner[k]))
    med = {k: statistics.median(v) for k, v in t.items()}
    rec = {"comparison": name, **extra, "rounds": rounds, "inner": inner,
           "ms": {k: round(1e3 * m, 4) for k, m in med.items()},
           "aa": {k: round(statistics.median(v[0::2]) / statistics.median(v[1::2]), 4) for k, v in t.items()},
           "min_ms": {k: round(1e3 * min(v), 4) for k, v in t.items()}, "max_ms": {k: round(1e3 * max(v), 4) for k, v in t.items()}}
    first = next(iter(arms))
    rec["over_" + first] = {k: round(med[k] / med[first], 4) for k in arms if k != first}
    print(json.dumps(rec), flush=True)
    return rec


def qr_like(seed):
    """A binary 300 x 300 watermark: 30 x 30 random modules of 10 x 10 pixels."""
    m = np.random.default_rng(seed).integers(0, 2, (30, 30), dtype=np.uint8) * 255
    return np.kron(m, np.ones((10, 10), np.uint8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--window", type=float, default=1.0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tile_ragged_time: no GPU (there is no CPU fallback to time)")
    dev = torch.device("cuda", 0)
    print(json.dumps({"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "window_s": a.window}), flush=True)
    b, alpha, n = 8, 0.1, 64
    rng = np.random.default_rng(20240)
    picks = [SIZES[int(k)] for k in rng.integers(0, len(SIZES), n)]  # ragged_bench's workload A
    sizes = [(h // b, w // b) for h, w in picks]
    wm_all = torch.from_numpy(np.stack([qr_like(8000 + i) for i in range(n)])).to(dev)
    wms = [wm_all[i] for i in range(n)]
    by_size = {}
    for i, s in enumerate(sizes):
        by_size.setdefault(s, []).append(i)
    stacks = {s: wm_all[idx].contiguous() for s, idx in by_size.items()}
    state = {}

    def loop():
        state["a"] = [batch.prepare_tile(w, th, tw, True) for w, (th, tw) in zip(wms, sizes)]

    def ragged():
        state["b"] = batch.prepare_tiles_ragged(wms, sizes, True)

    def grouped():
        state["c"] = {s: batch.prepare_tiles(stacks[s], s[0], s[1], True) for s in stacks}

    loop(), ragged(), grouped()
    torch.cuda.synchronize()
    for i in range(n):
        assert torch.equal(state["a"][i], state["b"][i]), ("ragged differs", i)
    for s, idx in by_size.items():
        for k, i in enumerate(idx):
            assert torch.equal(state["a"][i], state["c"][s][k]), ("grouped differs", i)
    info = {"jobs": n, "block": b, "preserve_ratio": True, "distinct_sizes": len(by_size), "outputs_equal": True}
    compare("workload A: tile preparation", {"a_64_prepare_tile": loop, "b_prepare_tiles_ragged": ragged, "c_5_prepare_tiles": grouped},
            a.rounds, a.window, info)

    frames = [batch.synth_photo_frames(1, h, w, seed=7000 + i, device=dev)[0].contiguous() for i, (h, w) in enumerate(picks)]
    outs = batch._ragged_views([f.numel() for f in frames], lambda i: frames[i].shape, dev)

    def e2e_loop():
        loop()
        batch.embed_ragged(frames, state["a"], b, alpha, out=outs)

    def e2e_ragged():
        ragged()
        batch.embed_ragged(frames, state["b"], b, alpha, out=outs)

    compare("workload A: tile preparation + embed_ragged", {"a_64_prepare_tile": e2e_loop, "b_prepare_tiles_ragged": e2e_ragged},
            a.rounds, a.window, {"jobs": n, "block": b, "megapixels": round(sum(h * w for h, w in picks) / 1e6, 1)})
    del frames, outs

    # 64 all-distinct tile sizes, no preserve_ratio: every job builds two axes of its own
    odd = [(40 + i, 110 + 3 * i) for i in range(n)]
    assert len({s[0] for s in odd} | {s[1] for s in odd}) == 2 * n

    def worst_loop():
        state["wa"] = [batch.prepare_tile(w, th, tw, False) for w, (th, tw) in zip(wms, odd)]

    def worst_ragged():
        state["wb"] = batch.prepare_tiles_ragged(wms, odd, False)

    worst_loop(), worst_ragged()
    torch.cuda.synchronize()
    for i in range(n):
        assert torch.equal(state["wa"][i], state["wb"][i]), ("worst case differs", i)
    compare("worst case: 128 distinct axes", {"a_64_prepare_tile": worst_loop, "b_prepare_tiles_ragged": worst_ragged}, a.rounds,
            a.window, {"jobs": n, "preserve_ratio": False, "distinct_axes": 2 * n, "outputs_equal": True})


if __name__ == "__main__":
    main()
