#!/usr/bin/env python3
"""Seeded CPU search for noise blocks whose key the embed strip pass cannot decide
(thatsmyface_amd/csrc/tmfwm_embed_key.h): certified blocks whose two pre-blend ends of sigma_1,
f32(sigma_1 -+ 2^-45 sigma_1), are two floats -- a float midpoint lies within 2^-45 sigma_1 of
the Jacobi route's f64 sigma_1.  About one noise block in 10^6.  The hits are tiled, among
ordinary noise blocks, into one small frame: the fixture tests/golden/embed_key_undecided_b<b>.npz
(frame, the hits' block positions, the seed, how many blocks were searched, how many hit).

usage: python tools/exp/embed_key_undecided.py --block 8 [--seed 20250] [--hits 6] [--max-blocks 40000000]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from embed_key_helpers import predict, predict_blocks  # noqa: E402
from oracle import oracle as O  # noqa: E402

CHUNK = 1 << 16
GRID = (4, 8)  # the fixture frame's block grid


def chunk_blocks(seed, i, b):
    """chunk i of the search: CHUNK noise blocks as (CHUNK, b, b, 3) u8"""
    return np.random.default_rng([seed, b, i]).integers(0, 256, (CHUNK, b, b, 3), dtype=np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--block", type=int, required=True)
    ap.add_argument("--seed", type=int, default=20250)
    ap.add_argument("--hits", type=int, default=6)
    ap.add_argument("--max-blocks", type=int, default=40_000_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    b = a.block
    out = a.out or os.path.join(ROOT, "tests", "golden", f"embed_key_undecided_b{b}.npz")
    found, searched, t0, i = [], 0, time.time(), 0
    while len(found) < a.hits and searched < a.max_blocks:
        rgb = chunk_blocks(a.seed, i, b)
        y = O.rgb_to_ycbcr(rgb.reshape(CHUNK * b, b, 3))[..., 0].reshape(CHUNK, b, b)
        cert, decided, _ = predict_blocks(O.dct2d_blocks(np.ascontiguousarray(y)))
        for k in np.flatnonzero(cert & ~decided):
            found.append(rgb[k].copy())
        searched += CHUNK
        i += 1
        if i % 16 == 0:
            print(f"{searched} blocks, {len(found)} hits, {time.time() - t0:.0f} s", flush=True)
    found = found[: a.hits]
    if not found:
        raise SystemExit(f"no hit in {searched} blocks")
    # the frame: noise blocks (the search's generator, chunk -1), the hits at spread positions
    nbh, nbw = GRID
    fill = np.random.default_rng([a.seed, b, 1 << 30]).integers(0, 256, (nbh, nbw, b, b, 3), dtype=np.uint8)
    at = [(int(p) // nbw, int(p) % nbw) for p in np.linspace(1, nbh * nbw - 2, len(found)).astype(int)]
    for (bi, bj), blk in zip(at, found):
        fill[bi, bj] = blk
    frame = np.ascontiguousarray(fill.transpose(0, 2, 1, 3, 4).reshape(nbh * b, nbw * b, 3))
    cert, decided, _ = predict(frame, b)
    und = cert & ~decided
    assert all(und[p] for p in at), "a tiled hit is decided: the search and the frame disagree"
    np.savez_compressed(out, frame=frame, undecided=np.argwhere(und).astype(np.int32), block=np.int32(b), seed=np.int64(a.seed),
                        blocks_searched=np.int64(searched), hits=np.int32(len(found)))
    print(f"b={b}: {len(found)} hits in {searched} blocks ({time.time() - t0:.0f} s), {int(und.sum())} undecided in the frame -> {out}")


if __name__ == "__main__":
    main()
