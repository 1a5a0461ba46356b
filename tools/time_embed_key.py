#!/usr/bin/env python3
"""Time embed-with-key against embed followed by the key map on synthetic 4K frames.

One process, HIP events, the arms alternating round by round on the same frames (tools/time_keyed.py's
frames and timer):
  embed_a, embed_b   batch.embed_batch(o, tile)                       embed alone, twice per round (A/A: the spread)
  embed_then_map     batch.embed_batch(o, tile); batch.sigma1_map(o)  both results the two-pass way
  embed_with_key     batch.embed_with_key(o, tile)                    both results from one call
Noise covers take a noise tile, camera-like covers the app's QR tile.  Before timing, the bytes and
key bits of the last two arms are compared.  Prints one JSON line per (block, kind): microseconds
per frame (median, min, max over the rounds), the A/A spread, and the fused call against both.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402
from time_keyed import covers, timed  # noqa: E402

from thatsmyface_amd import batch  # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--frames", type=int, default=128)
    p.add_argument("--height", type=int, default=2160)
    p.add_argument("--width", type=int, default=3840)
    p.add_argument("--blocks", type=int, nargs="+", default=[8, 16])
    p.add_argument("--kinds", nargs="+", choices=["noise", "photo"], default=["noise", "photo"])
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--reps", type=int, default=3, help="calls per timed window")
    p.add_argument("--route", choices=["hybrid", "reference", "rank1", "rank1_reference"], default="hybrid")
    p.add_argument("--out", help="also append the JSON lines to this file")
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_embed_key: no GPU (a timing needs one; there is no fallback)")
    dev = torch.device("cuda", 0)
    n, H, W, rt = a.frames, a.height, a.width, a.route
    for kind in a.kinds:
        o = covers(kind, n, H, W, dev)
        for b in a.blocks:
            nbh, nbw = H // b, W // b
            tile = batch.synth_tile(nbh, nbw, device=dev) if kind == "noise" else batch.synth_qr_tile(nbh, nbw, device=dev)
            se, sm, sk = {}, {}, {}
            w2 = batch.embed_batch(o, tile, b, 0.1, stats=se, route=rt)
            key2 = batch.sigma1_map(o, b, stats=sm, route=rt)
            w1, key1 = batch.embed_with_key(o, tile, b, 0.1, stats=sk, route=rt)
            same = bool(torch.equal(w1, w2)) and bool(torch.equal(key1.view(torch.int32), key2.view(torch.int32)))

            def two_pass():
                batch.embed_batch(o, tile, b, 0.1, out=w2, route=rt)
                batch.sigma1_map(o, b, out=key2, route=rt)

            arms = {
                "embed_a": lambda: batch.embed_batch(o, tile, b, 0.1, out=w2, route=rt),
                "embed_then_map": two_pass,
                "embed_with_key": lambda: batch.embed_with_key(o, tile, b, 0.1, out=w1, key_out=key1, route=rt),
                "embed_b": lambda: batch.embed_batch(o, tile, b, 0.1, out=w2, route=rt),
            }
            for fn in arms.values():  # warm-up: every timed shape once more
                fn()
            torch.cuda.synchronize()
            t = {k: [] for k in arms}
            for _ in range(a.rounds):
                for k, fn in arms.items():
                    t[k].append(timed(fn, a.reps) / n)
            med = {k: statistics.median(v) for k, v in t.items()}
            emb = 0.5 * (med["embed_a"] + med["embed_b"])
            line = {
                "block": b, "kind": kind, "route": rt, "frames": n, "size": [H, W], "rounds": a.rounds, "reps": a.reps,
                "bytes_and_key_bits_equal": same,
                "us_per_frame": {k: {"median": round(med[k], 2), "min": round(min(v), 2), "max": round(max(v), 2)} for k, v in t.items()},
                "aa_spread": round(abs(med["embed_a"] - med["embed_b"]) / emb, 4),
                "embed_round_spread": round((max(t["embed_a"] + t["embed_b"]) - min(t["embed_a"] + t["embed_b"])) / emb, 4),
                "with_key_over_embed_then_map": round(med["embed_with_key"] / med["embed_then_map"], 4),
                "with_key_minus_embed_us": round(med["embed_with_key"] - emb, 2),
                "embed_then_map_minus_embed_us": round(med["embed_then_map"] - emb, 2),
                "dgesdd_route_blocks": {"embed": se["lapack_blocks"], "map": sm["lapack_blocks"], "embed_with_key": sk["lapack_blocks"]},
                "list_pass_blocks": {"embed": se["list_pass_blocks"], "map": sm["list_pass_blocks"], "embed_with_key": sk["list_pass_blocks"]},
            }
            s = json.dumps(line)
            print(s, flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(s + "\n")
            if not same:
                sys.exit("time_embed_key: the fused call's bytes or key bits differ from embed + map")
            del w1, w2, key1, key2
        del o
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
