#!/usr/bin/env python3
"""Time keyed extraction against the pair path on synthetic 4K frames.

One process, HIP events, the variants alternating round by round on the same frames:
  pair_a, pair_b   batch.extract_batch(w, o)            the pair path, twice per round (A/A: the spread)
  keyed            batch.extract_keyed(w, key)          key made once, outside the timed window
  map              batch.sigma1_map(o)
Before timing, the keyed bytes are compared with the pair path's.  Prints one JSON line per
(block, kind): microseconds per frame (median, min, max over the rounds), the A/A spread, and
the ratios keyed / pair and (map + keyed) / pair.

--pixel-bytes 4 adds, in the same rounds, the two ways a holder of R G B pad frames has:
  keyed4, map4            the same calls on the (N, H, W, 4) frames, read in place
  keyed_pack, map_pack    frames[..., :3].contiguous() and then the 3-byte call (what such a holder
                          had to do before the keyed calls took 4-byte frames)
and their ratios (in place / 3-byte, in place / pack-then-call).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from thatsmyface_amd import batch  # noqa: E402


def covers(kind, n, H, W, dev):
    if kind == "noise":
        return batch.synth_frames(n, H, W, device=dev)
    sys.path.insert(0, os.path.join(ROOT, "tools", "exp"))
    from route_diff_gpu import photo_covers

    # in groups: the recipe's f32 intermediates are 4 bytes per sample
    return torch.cat([photo_covers(min(16, n - i), H, W, 5 + i, dev) for i in range(0, n, 16)])


def rgbx(frames):
    """(N, H, W, 3) -> (N, H, W, 4): the same R, G, B and a pad byte of 255"""
    out = torch.full(frames.shape[:3] + (4,), 255, dtype=torch.uint8, device=frames.device)
    out[..., :3] = frames
    return out


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / reps  # us per call


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
    p.add_argument("--pixel-bytes", type=int, choices=[3, 4], default=3, help="4: also time the keyed calls on R G B pad frames")
    p.add_argument("--out", help="also append the JSON lines to this file")
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_keyed: no GPU (a timing needs one; there is no fallback)")
    dev = torch.device("cuda", 0)
    n, H, W, rt = a.frames, a.height, a.width, a.route
    for kind in a.kinds:
        o = covers(kind, n, H, W, dev)
        for b in a.blocks:
            tile = batch.synth_tile(H // b, W // b, device=dev)
            w = batch.embed_batch(o, tile, b, 0.1)
            sp, sk, sm = {}, {}, {}
            key = batch.sigma1_map(o, b, stats=sm, route=rt)
            ext_p = batch.extract_batch(w, o, b, 0.1, stats=sp, route=rt)
            ext_k = batch.extract_keyed(w, key, b, 0.1, stats=sk, route=rt)
            same = bool(torch.equal(ext_p, ext_k))
            variants = {
                "pair_a": lambda: batch.extract_batch(w, o, b, 0.1, out=ext_p, route=rt),
                "keyed": lambda: batch.extract_keyed(w, key, b, 0.1, out=ext_k, route=rt),
                "map": lambda: batch.sigma1_map(o, b, out=key, route=rt),
                "pair_b": lambda: batch.extract_batch(w, o, b, 0.1, out=ext_p, route=rt),
            }
            if a.pixel_bytes == 4:
                o4, w4 = rgbx(o), rgbx(w)
                key4, ext4 = torch.empty_like(key), torch.empty_like(ext_k)
                batch.sigma1_map(o4, b, out=key4, route=rt)
                batch.extract_keyed(w4, key, b, 0.1, out=ext4, route=rt)
                same = same and bool(torch.equal(ext4, ext_k)) and bool(torch.equal(key4.view(torch.int32), key.view(torch.int32)))
                variants.update({
                    "keyed4": lambda: batch.extract_keyed(w4, key, b, 0.1, out=ext4, route=rt),
                    "map4": lambda: batch.sigma1_map(o4, b, out=key4, route=rt),
                    "keyed_pack": lambda: batch.extract_keyed(w4[..., :3].contiguous(), key, b, 0.1, out=ext4, route=rt),
                    "map_pack": lambda: batch.sigma1_map(o4[..., :3].contiguous(), b, out=key4, route=rt),
                })
            for fn in variants.values():  # warm-up: every timed shape once more
                fn()
            torch.cuda.synchronize()
            t = {k: [] for k in variants}
            for _ in range(a.rounds):
                for k, fn in variants.items():
                    t[k].append(timed(fn, a.reps) / n)
            med = {k: statistics.median(v) for k, v in t.items()}
            pair = 0.5 * (med["pair_a"] + med["pair_b"])
            line = {
                "block": b, "kind": kind, "route": rt, "frames": n, "size": [H, W], "rounds": a.rounds, "reps": a.reps,
                "bytes_equal": same,
                "us_per_frame": {k: {"median": round(med[k], 2), "min": round(min(v), 2), "max": round(max(v), 2)} for k, v in t.items()},
                "aa_spread": round(abs(med["pair_a"] - med["pair_b"]) / pair, 4),
                "pair_round_spread": round((max(t["pair_a"] + t["pair_b"]) - min(t["pair_a"] + t["pair_b"])) / pair, 4),
                "keyed_over_pair": round(med["keyed"] / pair, 4),
                "map_plus_keyed_over_pair": round((med["map"] + med["keyed"]) / pair, 4),
                "dgesdd_route_blocks": {"pair": sp["lapack_blocks"], "keyed": sk["lapack_blocks"], "map": sm["lapack_blocks"]},
                "list_pass_blocks": {"pair": sp["list_pass_blocks"], "keyed": sk["list_pass_blocks"], "map": sm["list_pass_blocks"]},
            }
            if a.pixel_bytes == 4:
                line["keyed_round_spread"] = round((max(t["keyed"]) - min(t["keyed"])) / med["keyed"], 4)
                line["map_round_spread"] = round((max(t["map"]) - min(t["map"])) / med["map"], 4)
                for k in ("keyed", "map"):
                    line[k + "4_over_" + k] = round(med[k + "4"] / med[k], 4)
                    line[k + "4_over_" + k + "_pack"] = round(med[k + "4"] / med[k + "_pack"], 4)
                del o4, w4, key4, ext4
            s = json.dumps(line)
            print(s, flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(s + "\n")
            if not same:
                sys.exit("time_keyed: keyed bytes differ from the pair path")
            del w, key, ext_p, ext_k
        del o
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
