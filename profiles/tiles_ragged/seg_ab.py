"""Workload A's 64 jobs: 3 warm-up calls + 20 calls of prepare_tiles_ragged (kernel stats under rocprofv3; TMFWM_LIB picks the build)."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
from thatsmyface_amd import batch
from tools.ragged_bench import SIZES
from tools.tile_ragged_time import qr_like

dev = torch.device("cuda", 0)
rng = np.random.default_rng(20240)
picks = [SIZES[int(k)] for k in rng.integers(0, len(SIZES), 64)]
sizes = [(h // 8, w // 8) for h, w in picks]
wm_all = torch.from_numpy(np.stack([qr_like(8000 + i) for i in range(64)])).to(dev)
wms = [wm_all[i] for i in range(64)]
for _ in range(3):
    tiles = batch.prepare_tiles_ragged(wms, sizes, True)
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(20):
    tiles = batch.prepare_tiles_ragged(wms, sizes, True)
torch.cuda.synchronize()
ref = [batch.prepare_tile(w, th, tw, True) for w, (th, tw) in zip(wms, sizes)]
assert all(torch.equal(a, b) for a, b in zip(tiles, ref))
print("lib", os.environ.get("TMFWM_LIB", "product"), "wall ms/call", round((time.perf_counter() - t0) / 20 * 1e3, 4))
