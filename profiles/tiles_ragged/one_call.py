"""One tmfwm_prepare_tiles_ragged call on workload A's 64 jobs, for a kernel / copy trace."""
import os, sys
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
wm_all = torch.from_numpy(np.stack([qr_like(8000 + i) for i in range(64)])).to(dev)  # the one upload that is not the call's
wms = [wm_all[i] for i in range(64)]
torch.cuda.synchronize()
tiles = batch.prepare_tiles_ragged(wms, sizes, True)
torch.cuda.synchronize()
print("tiles", len(tiles), "bytes", sum(t.numel() for t in tiles))
