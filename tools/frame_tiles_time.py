"""What per-frame tiles buy: device-event timings on warmed-up work of at least a second."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from thatsmyface_amd import batch

dev = torch.device("cuda", 0)
n, H, W, b = 256, 1080, 1920, 8
nbh, nbw = H // b, W // b
frames = batch.synth_frames(n, H, W, device=dev)
out = torch.empty_like(frames)
wms = torch.from_numpy(np.random.default_rng(1).integers(0, 2, (n, 300, 300), dtype=np.uint8) * 255).to(dev)
tiles = batch.prepare_tiles(wms, nbh, nbw, True)
shared = tiles[0].contiguous()


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def per_image():
    for i in range(n):
        t = batch.prepare_tile(wms[i], nbh, nbw, True)
        batch.embed_batch(frames[i:i + 1], t, b, 0.1, out=out[i:i + 1])


def batched():
    t = batch.prepare_tiles(wms, nbh, nbw, True)
    batch.embed_batch(frames, t, b, 0.1, out=out)


def prep_loop():
    for i in range(n):
        batch.prepare_tile(wms[i], nbh, nbw, True)


res = {"frames": n, "height": H, "width": W, "block": b}
for rnd in range(2):  # alternate, twice
    res[f"embed_shared_ms_{rnd}"] = timed(lambda: batch.embed_batch(frames, shared, b, 0.1, out=out), 150)
    res[f"embed_per_frame_ms_{rnd}"] = timed(lambda: batch.embed_batch(frames, tiles, b, 0.1, out=out), 150)
for rnd in range(2):
    res[f"one_call_per_image_ms_{rnd}"] = timed(per_image, 12)
    res[f"prepare_tiles_plus_one_embed_ms_{rnd}"] = timed(batched, 120)
for rnd in range(2):
    res[f"prepare_tile_x256_ms_{rnd}"] = timed(prep_loop, 30)
    res[f"prepare_tiles_256_ms_{rnd}"] = timed(lambda: batch.prepare_tiles(wms, nbh, nbw, True), 1500)
print(json.dumps(res))
