"""Job list of the ragged tile-preparation tests (tests/test_tiles_ragged.py on the CPU,
tests/test_tiles_ragged_gpu.py on the GPU): the smallest shapes that reach each index path of
tmfwm_prepare_tiles_ragged.  Expected tiles always come from the oracle's prepare_tile."""
import functools

import numpy as np

from oracle import oracle as O

# (watermark (h, w), tile (h, w))
JOBS = [
    ((300, 300), (2, 3)),      # support wider than the input: every tap row spans the whole watermark
    ((300, 300), (17, 25)),    # strong downscale; with ratio a 17 x 17 paste at px = 4
    ((300, 300), (60, 80)),    # twice, different bytes: one plan, two data sets
    ((300, 300), (60, 80)),
    ((29, 31), (17, 25)),      # non-square; with ratio resized to (17, 18)
    ((29, 31), (29, 31)),      # copy: neither pass
    ((29, 31), (40, 31)),      # vertical only; with ratio a copy pasted at py = 5
    ((29, 31), (29, 50)),      # horizontal only
    ((17, 25), (135, 240)),    # upscale on both axes; with ratio (135, 198) pasted at px = 21
    ((29, 31), (3, 300)),      # a row wider than one segment, 64 or 256 bytes
]
# valid without preserve_ratio; with it the resized size is empty
ERROR_JOBS = [((1, 700), (5, 3)), ((700, 1), (3, 5))]


@functools.lru_cache(maxsize=None)
def watermarks():
    """One watermark per job: random bytes for even jobs, binary 0 / 255 (QR-like) for odd ones."""
    out = []
    for i, (shape, _) in enumerate(JOBS):
        a = np.random.default_rng(7000 + i).integers(0, 256, shape, dtype=np.uint8)
        out.append(a if i % 2 == 0 else ((a & 1) * 255).astype(np.uint8))
    assert not np.array_equal(out[2], out[3])
    return tuple(out)


@functools.lru_cache(maxsize=None)
def expected(preserve_ratio: bool):
    return tuple(O.prepare_tile(w, th, tw, preserve_ratio) for w, (_, (th, tw)) in zip(watermarks(), JOBS))


def resized(wm, tile, preserve_ratio):
    """resize_watermark's resized size (watermarking.py:105-110)."""
    (wh, ww), (th, tw) = wm, tile
    if not preserve_ratio:
        return th, tw
    ratio = min(tw / ww, th / wh)
    return int(wh * ratio), int(ww * ratio)


def distinct_axes(preserve_ratio: bool) -> int:
    """The distinct (input size, output size) pairs of the list, both directions together."""
    pairs = set()
    for wm, tile in JOBS:
        rh, rw = resized(wm, tile, preserve_ratio)
        pairs.add((wm[1], rw))
        pairs.add((wm[0], rh))
    return len(pairs)
