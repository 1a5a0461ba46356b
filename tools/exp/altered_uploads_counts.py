#!/usr/bin/env python3
"""Altered uploads (tests/upload_classes.py): what the GPU's extract sends to the list pass and to
the dgesdd route, per block size, cover and class, next to the bounds of the numpy model of the
sigma_1 enclosure (tests/sigma1_helpers.py).  Writes profiles/altered_uploads/results.json (or the
path given as the first argument).

Per class one extract_batch call of one frame pair on the hybrid route ("pair": lapack_blocks,
list_pass_blocks) and one extract_ragged call ("ragged": no list pass runs, so lapack_blocks is
what the strip pass left).  Model, over EITHER image of the pair: "never" (2 sigma_1^2 <= F, no
vector decides), "list" (undecided by an enclosure twice the model's width after the list pass's
iterations) and "strip" (undecided by the model after the strip pass's iterations).  Expected:
never <= pair.lapack_blocks <= list, pair.list_pass_blocks <= strip, never <= ragged.lapack_blocks
<= strip.  A count outside its bound is listed under "findings" with the model's blocks nearest
their decision (distance of LAPACK's sigma_1 from a float midpoint, in units of 2^-53 sigma_1)."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import sigma1_helpers as S  # noqa: E402
import upload_classes as UC  # noqa: E402

from thatsmyface_amd import batch  # noqa: E402


def nearest_blocks(frame, b, k=3):
    """The k blocks of a frame nearest a float midpoint: [[row, col, units], ...]."""
    D = S.frame_blocks(frame, b)
    dist = S.midpoint_distance(S.sigma1_lapack(D))
    nbw = frame.shape[1] // b
    return [[int(i // nbw), int(i % nbw), float(dist[i])] for i in np.argsort(dist)[:k]]


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "altered_uploads", "results.json")
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "embed_alpha": UC.EMBED_ALPHA, "extract_alpha": 0.1,
           "frame": "(6b+3) x (70b+5) pixels", "sizes": {}, "findings": []}
    for b in UC.BLOCKS:
        per_b = res["sizes"][f"b{b}"] = {}
        for kind in ("photo", "noise", "qr"):
            cp = UC.corpus(b, kind)
            cnt = cp.counts
            per_k = per_b[kind] = {"blocks_per_frame": int(cp.keys_up[0].size), "classes": {}}
            for i, name in enumerate(cp.names):
                u = torch.from_numpy(np.array(cp.up[i:i + 1], copy=True)).to(dev)
                o = torch.from_numpy(np.array(cp.orig[i:i + 1], copy=True)).to(dev)
                sp, sr = {}, {}
                got = batch.extract_batch(u, o, b, 0.1, stats=sp)[0].cpu().numpy()
                rag = batch.extract_ragged([u[0]], [o[0]], b, 0.1, stats=sr)[0].cpu().numpy()
                model = {k: int(cnt[k][i].sum()) for k in ("never", "list", "strip")}
                ok_bytes = bool(np.array_equal(got, cp.expect(0.1)[i]) and np.array_equal(rag, cp.expect(0.1)[i]))
                per_k["classes"][name] = {"pair": sp, "ragged": {"lapack_blocks": sr["lapack_blocks"]}, "model": model,
                                          "bytes_equal_oracle": ok_bytes}
                within = (model["never"] <= sp["lapack_blocks"] <= model["list"] and sp["list_pass_blocks"] <= model["strip"]
                          and model["never"] <= sr["lapack_blocks"] <= model["strip"])
                if not (within and ok_bytes):
                    res["findings"].append({"block": b, "cover": kind, "class": name, "pair": sp, "ragged": sr, "model": model,
                                            "bytes_equal_oracle": ok_bytes,
                                            "nearest_midpoint_upload": nearest_blocks(cp.up[i], b),
                                            "nearest_midpoint_original": nearest_blocks(cp.orig[i], b)})
            print(f"b={b} {kind}: " + ", ".join(f"{n} {c['pair']['lapack_blocks']}/{c['pair']['list_pass_blocks']}/{c['ragged']['lapack_blocks']}"
                                                f" (<= {c['model']['list']}/{c['model']['strip']}/{c['model']['strip']})"
                                                for n, c in per_k["classes"].items()), flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(f"wrote {out_path}: {len(res['findings'])} findings")


if __name__ == "__main__":
    main()
