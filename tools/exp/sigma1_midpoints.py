#!/usr/bin/env python3
"""Seeded CPU search for blocks whose sigma_1 lies next to a midpoint between two floats, the only
blocks at which the margins of the extract path's sigma_1 enclosure (sigma1_certified)
decide anything.  tests/sigma1_helpers.py defines the classes:

  must refuse  LAPACK's sigma_1 closer than 600 units of 2^-53 sigma_1 to a midpoint;
  must keep    600 .. 20480 units away, decided by an enclosure twice as wide as the numpy model's;
  fill         at least 2^-36 sigma_1 away, decided by that widened enclosure.

The search walks a fixed number of chunks -- three of 65536 uniform-noise blocks, then one of 16384
blocks cut from four lapack_path.photo_cover frames, and so on -- so its result does not depend
on how many processes share the work.  About 1.5 to 3 blocks per million are must-refuse ones.  Up
to 8 of them (at least 6, at least 2 further than 200 units from the midpoint, a photo-cover one
first if one turned up) and the 12 must-keep blocks nearest to a midpoint are tiled among fill
blocks (16-level noise and photo-cover ones alternating) into one 4 x 16 block frame: the fixture
tests/golden/sigma1_midpoints_b<b>.npz (frame, positions and distances of both classes, which
must-refuse blocks are photo-cover ones, the seed, the number of blocks searched).  A hit closer
than 8 units to a class bound is passed over, so that another LAPACK build's last bits cannot move
a fixture block into another class.

Budget used for the committed fixtures: the default, 256 chunks = 13.6 M blocks per block size
(10 s at b = 4 to about a minute at b = 16, on 8 processes).

usage: python tools/exp/sigma1_midpoints.py --block 8 [--seed 20251] [--chunks 256] [--procs 8]"""
import argparse
import multiprocessing as mp
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sigma1_helpers as S  # noqa: E402
from lapack_path import photo_cover  # noqa: E402
from oracle import oracle as O  # noqa: E402

NOISE_CHUNK = 1 << 16
PHOTO_SIDE = 64  # a photo-cover frame is 64 x 64 blocks; a photo chunk is four frames
GRID = (4, 16)  # the fixture frame's block grid
MAX_REFUSE, N_KEEP = 8, 12
GUARD = 8.0  # units kept clear of every class bound


def is_photo(i):
    return i % 4 == 3


def chunk_blocks(seed, i, b):
    """chunk i of the search as (n, b, b, 3) u8 blocks"""
    if not is_photo(i):
        return np.random.default_rng([seed, b, i]).integers(0, 256, (NOISE_CHUNK, b, b, 3), dtype=np.uint8)
    side = PHOTO_SIDE * b
    frames = [photo_cover(side, side, seed + 1000 * i + k) for k in range(4)]
    return np.concatenate([f.reshape(PHOTO_SIDE, b, PHOTO_SIDE, b, 3).transpose(0, 2, 1, 3, 4).reshape(-1, b, b, 3) for f in frames])


def dct_of(rgb):
    n, b = rgb.shape[:2]
    y = O.rgb_to_ycbcr(np.ascontiguousarray(rgb).reshape(n * b, b, 3))[..., 0].reshape(n, b, b)
    return O.dct2d_blocks(np.ascontiguousarray(y))


def scan(job):
    """the candidates of one chunk: (chunk, index, class, distance, block)"""
    seed, i, b = job
    rgb = chunk_blocks(seed, i, b)
    D = dct_of(rgb)
    # screen with singular values alone (they differ from the full factorisation's by a few units)
    near = np.flatnonzero(S.midpoint_distance(np.linalg.svd(D.astype(np.float64), compute_uv=False)[:, 0]) < S.KEEP_MAX + 64)
    out = []
    if len(near):
        cls, dist, _ = S.classify(D[near])
        for k, c, d in zip(near, cls, dist):
            clear = min(abs(d - S.REFUSE), abs(d - S.KEEP_MAX)) >= GUARD
            if clear and c in (S.MUST_REFUSE, S.MUST_KEEP):
                out.append((i, int(k), int(c), float(d), rgb[k].copy()))
    return len(rgb), out


def fill_blocks(seed, b, n):
    """n fill-class blocks, noise and photo-cover ones alternating; the noise takes 16 grey levels
    only, which keeps the largest fixture below 50 KB"""
    rng = np.random.default_rng([seed, b, 1 << 30])
    noise = (17 * rng.integers(0, 16, (4 * n, b, b, 3))).astype(np.uint8)
    side = 16 * b
    photo = photo_cover(side, side, seed + 7).reshape(16, b, 16, b, 3).transpose(0, 2, 1, 3, 4).reshape(-1, b, b, 3)
    pools = []
    for pool in (noise, photo):
        cls, dist, _ = S.classify(dct_of(pool))
        pools.append(list(pool[(cls == S.FILL) & (dist >= S.FILL_MIN + 64)]))
    return [pools[k % 2].pop(0) for k in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--block", type=int, required=True)
    ap.add_argument("--seed", type=int, default=20251)
    ap.add_argument("--chunks", type=int, default=256)
    ap.add_argument("--procs", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    b = a.block
    out = a.out or os.path.join(ROOT, "tests", "golden", f"sigma1_midpoints_b{b}.npz")
    t0, searched, hits = time.time(), 0, []
    with mp.Pool(a.procs) as pool:
        for n, found in pool.imap(scan, [(a.seed, i, b) for i in range(a.chunks)]):  # in chunk order
            searched += n
            hits += found
    refuse = [h for h in hits if h[2] == S.MUST_REFUSE]
    keep = sorted((h for h in hits if h[2] == S.MUST_KEEP), key=lambda h: h[3])[:N_KEEP]
    print(f"b={b}: {searched} blocks, {len(refuse)} must-refuse ({sum(is_photo(h[0]) for h in refuse)} photo), "
          f"{sum(h[2] == S.MUST_KEEP for h in hits)} must-keep, {time.time() - t0:.0f} s", flush=True)
    # photo-cover hits first, then those further than 200 units out, then search order
    ids = list(range(len(refuse)))
    first = [k for k in ids if is_photo(refuse[k][0])][:1]
    far = [k for k in ids if k not in first and refuse[k][3] > 200.0][:2]
    pick = (first + far + [k for k in ids if k not in first + far])[:MAX_REFUSE]
    refuse = [refuse[k] for k in sorted(pick)]
    if len(refuse) < 6 or sum(h[3] > 200.0 for h in refuse) < 2 or len(keep) < N_KEEP:
        raise SystemExit(f"too few hits in {searched} blocks: raise --chunks")
    nbh, nbw = GRID
    rng = np.random.default_rng([a.seed, b, 1 << 29])
    while True:  # must-refuse blocks in both halves of the frame (the ragged tests cut the top half off)
        at = [(int(p) // nbw, int(p) % nbw) for p in rng.permutation(nbh * nbw)]
        top = sum(r < nbh // 2 for r, _ in at[: len(refuse)])
        if 2 <= top <= len(refuse) - 2:
            break
    listed = refuse + keep
    grid = np.empty((nbh, nbw, b, b, 3), np.uint8)
    for pos, blk in zip(at, [h[4] for h in listed] + fill_blocks(a.seed, b, nbh * nbw - len(listed))):
        grid[pos] = blk
    frame = np.ascontiguousarray(grid.transpose(0, 2, 1, 3, 4).reshape(nbh * b, nbw * b, 3))
    cls, dist, _ = S.classify_frame(frame, b)
    r_at, k_at = at[: len(refuse)], at[len(refuse): len(listed)]
    assert all(cls[p] == S.MUST_REFUSE for p in r_at) and all(cls[p] == S.MUST_KEEP for p in k_at), "the search and the frame disagree"
    assert int((cls == S.FILL).sum()) == nbh * nbw - len(listed), "a fill block is of no class"
    order_r, order_k = sorted(range(len(r_at)), key=lambda k: r_at[k]), sorted(range(len(k_at)), key=lambda k: k_at[k])
    np.savez_compressed(
        out, frame=frame, block=np.int32(b), seed=np.int64(a.seed), blocks_searched=np.int64(searched),
        refuse=np.array([r_at[k] for k in order_r], np.int32), refuse_units=np.array([dist[r_at[k]] for k in order_r]),
        refuse_photo=np.array([is_photo(refuse[k][0]) for k in order_r]),
        keep=np.array([k_at[k] for k in order_k], np.int32), keep_units=np.array([dist[k_at[k]] for k in order_k]))
    print(f"b={b}: {len(r_at)} must-refuse at {sorted(r_at)}, units {np.round(sorted(dist[p] for p in r_at), 1).tolist()}; "
          f"{len(k_at)} must-keep, units {np.round(sorted(dist[p] for p in k_at)).tolist()} -> {out} ({os.path.getsize(out)} bytes)")


if __name__ == "__main__":
    main()
