"""Batched app pipeline for the embed page.

The reference page embeds uploaded images one at a time
(internal_pages/embed_watermark_page.py:492-558): PIL decode, ``embed_watermark``,
PNG encode into session state, then ``time.sleep(0.1)``.  Once the watermark
arithmetic runs on the GPU, the per-image decode / encode on one host thread is
what is left.  This module overlaps the three stages:

* decode (thread pool): ``Image.open(...).convert("RGB")`` -> uint8 array;
* device (one ordered stage): pinned host buffer -> async H2D on a side stream ->
  ``embed_batch`` (one launch) -> async D2H into pinned memory; the watermark tile
  for each image size is prepared once on the device (``tmfwm_prepare_tile``);
  with ``batch_images=K`` the stage takes up to K decoded images of any sizes at a time and
  prepares the group's tiles with one ``prepare_tiles_ragged`` and embeds the group with one
  ``embed_ragged`` (``RaggedGpuStage``);
* encode (thread pool): waits for the copy, PNG-encodes (zlib releases the GIL).

Results come back in input order and are byte-identical to
``embed_watermark(img, watermark_data, preserve_ratio)`` followed by
``img.save(format="PNG")`` per image.  The device stage is a parameter so the
pipeline logic is testable on CPU (tests/test_pipeline.py).
"""
from __future__ import annotations

import io
import os
from concurrent.futures import Future, ThreadPoolExecutor
from dataclasses import dataclass
from typing import Callable, Iterable, Sequence

import numpy as np
from PIL import Image

from .constants import ALPHA, BLOCK_SIZE, SVD_ROUTE


@dataclass
class Embedded:
    """One pipeline result: the watermarked RGB pixels and their PNG encoding."""

    pixels: np.ndarray
    png: bytes

    def image(self) -> Image.Image:
        return Image.fromarray(self.pixels, "RGB")


def _decode(src) -> np.ndarray:
    img = src if isinstance(src, Image.Image) else Image.open(io.BytesIO(src) if isinstance(src, (bytes, bytearray)) else src)
    return np.ascontiguousarray(np.asarray(img.convert("RGB"), dtype=np.uint8))


def _encode(pixels: np.ndarray, wait: Callable[[], None] | None) -> Embedded:
    if wait is not None:
        wait()
    buf = io.BytesIO()
    Image.fromarray(pixels, "RGB").save(buf, format="PNG")  # embed_watermark_page.py:533-535
    return Embedded(pixels, buf.getvalue())


class GpuStage:
    """Device stage: per image, pinned staging + side-stream H2D / embed / D2H.

    Returns (pixels, wait) where ``wait()`` blocks until the D2H copy landed.  The
    tile for an image size is prepared on the device once and reused.  ``watermark_data``
    may be a list or tuple of watermarks, one per image: the stage is then called as
    ``stage(rgb, i)`` and keeps its per-size tile cache per watermark."""

    def __init__(self, watermark_data, block: int, alpha: float, preserve_ratio: bool, device=None, route: str = SVD_ROUTE):
        import torch

        from . import batch

        self.torch, self.batch = torch, batch
        self.block, self.alpha, self.preserve_ratio = int(block), float(alpha), bool(preserve_ratio)
        self.route = route  # the drop-in's SVD route (constants.SVD_ROUTE, custom_settings["svd_route"])
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.per_image = isinstance(watermark_data, (list, tuple))
        self.wm_grey = []  # one grey watermark on the device per watermark
        for data in (watermark_data if self.per_image else [watermark_data]):
            wm = data if isinstance(data, Image.Image) else Image.open(io.BytesIO(data))
            grey = np.array(wm.convert("L"), dtype=np.uint8, copy=True)  # watermarking.py:98-103
            self.wm_grey.append(torch.from_numpy(grey).to(self.device))
        self.stream = torch.cuda.Stream(device=self.device)
        self.tiles: dict[tuple[int, int, int], object] = {}  # (watermark, nbh, nbw) -> tile

    def _tile(self, nbh: int, nbw: int, index: int = 0):
        key = (index, nbh, nbw)
        if key not in self.tiles:
            with self.torch.cuda.stream(self.stream):
                self.tiles[key] = self.batch.prepare_tile(self.wm_grey[index], nbh, nbw, self.preserve_ratio, stream=self.stream)
        return self.tiles[key]

    def __call__(self, rgb: np.ndarray, index: int = 0):
        torch = self.torch
        h, w = rgb.shape[:2]
        nbh, nbw = h // self.block, w // self.block
        if nbh == 0 or nbw == 0:
            raise ValueError("height and width must be > 0")  # PIL's resize raises in the reference
        host_in = torch.empty((1, h, w, 3), dtype=torch.uint8, pin_memory=True)
        host_in.numpy()[0] = rgb
        host_out = torch.empty((1, h, w, 3), dtype=torch.uint8, pin_memory=True)
        tile = self._tile(nbh, nbw, index)
        with torch.cuda.stream(self.stream):
            dev_in = host_in.to(self.device, non_blocking=True)
            dev_out = self.batch.embed_batch(dev_in, tile, self.block, self.alpha, stream=self.stream, route=self.route)
            host_out.copy_(dev_out, non_blocking=True)
            done = torch.cuda.Event()
            done.record(self.stream)
        # keep the device buffers alive until the copy has landed
        keep = (dev_in, dev_out, host_in)

        def wait(_e=done, _k=keep):
            _e.synchronize()

        return host_out.numpy()[0], wait


class RaggedGpuStage(GpuStage):
    """Batched device stage (``embed_images(..., batch_images=K)``): a group of decoded images of
    any sizes is uploaded, one ``prepare_tiles_ragged`` makes the tiles the group needs and the
    cache does not hold, one ``embed_ragged`` embeds the whole group, and the results are copied
    back.

    Called as ``stage(rgbs, indices)`` with the group's pixel arrays and their positions in the
    input (the watermark of image ``i`` is watermark ``i`` when there is one per image); returns
    one ``(pixels, wait)`` per image, in the group's order."""

    def _group_tiles(self, keys):
        """The tiles of a group's (watermark, nbh, nbw) keys: those the cache does not hold, each
        once, from one ``prepare_tiles_ragged`` on the stage's stream (no synchronisation).  With
        one watermark for all images a size's tile stays cached for later groups; with one
        watermark per image a key is used once, so its tile lives only as long as the group."""
        need = [k for k in dict.fromkeys(keys) if k not in self.tiles]
        made = {}
        if need:
            made = dict(zip(need, self.batch.prepare_tiles_ragged([self.wm_grey[k[0]] for k in need], [k[1:] for k in need],
                                                                  self.preserve_ratio, stream=self.stream)))
            if not self.per_image:
                self.tiles.update(made)
        return [made[k] if k in made else self.tiles[k] for k in keys]

    def __call__(self, rgbs, indices):
        torch = self.torch
        keys, host_in, host_out = [], [], []
        for rgb, index in zip(rgbs, indices):
            h, w = rgb.shape[:2]
            nbh, nbw = h // self.block, w // self.block
            if nbh == 0 or nbw == 0:
                raise ValueError("height and width must be > 0")  # as GpuStage
            keys.append((index if self.per_image else 0, nbh, nbw))
            hi = torch.empty((h, w, 3), dtype=torch.uint8, pin_memory=True)
            hi.numpy()[...] = rgb
            host_in.append(hi)
            host_out.append(torch.empty((h, w, 3), dtype=torch.uint8, pin_memory=True))
        with torch.cuda.stream(self.stream):
            tiles = self._group_tiles(keys)
            dev_in = [h.to(self.device, non_blocking=True) for h in host_in]
            dev_out = self.batch.embed_ragged(dev_in, tiles, self.block, self.alpha, stream=self.stream, route=self.route)
            for ho, do in zip(host_out, dev_out):
                ho.copy_(do, non_blocking=True)
            done = torch.cuda.Event()
            done.record(self.stream)
        keep = (dev_in, dev_out, host_in, tiles)  # alive until the copies have landed

        def wait(_e=done, _k=keep):
            _e.synchronize()

        return [(ho.numpy(), wait) for ho in host_out]


def embed_images(images: Iterable, watermark_data, preserve_ratio: bool = True, custom_settings: dict | None = None,
                 workers: int | None = None, device_stage: Callable | None = None,
                 batch_images: int | None = None) -> list[Embedded]:
    """Embed ``watermark_data`` (PNG bytes or PIL image) into every image (bytes, file
    object or PIL image) -- embed_watermark_page.py:492-558 without the per-image
    serialisation.  Returns, in input order, the watermarked pixels and PNG bytes.

    ``watermark_data`` may also be a list or tuple with one watermark per image (a service
    watermarking many users' images: no two QR codes are alike): image i gets watermark i, a
    length mismatch raises ValueError, and a custom ``device_stage`` is called as
    ``stage(rgb, i)`` instead of ``stage(rgb)``.

    ``batch_images=K`` makes the device stage take up to K decoded images at a time, of any
    sizes, and embed each group with one ragged launch set (``RaggedGpuStage``; a custom
    ``device_stage`` is then called as ``stage(rgbs, indices)`` and returns one
    ``(pixels, wait)`` per image).  Order, pixels and PNG bytes are those of the per-image path,
    which ``None`` keeps."""
    settings = custom_settings or {}
    block = int(settings.get("block_size", BLOCK_SIZE))
    alpha = float(settings.get("alpha", ALPHA))
    route = settings.get("svd_route") or os.environ.get("TMFWM_SVD_ROUTE") or SVD_ROUTE  # as watermarking._route
    sources: Sequence = list(images)
    per_image = isinstance(watermark_data, (list, tuple))
    if per_image and len(watermark_data) != len(sources):
        raise ValueError(f"{len(watermark_data)} watermarks for {len(sources)} images")
    if batch_images is not None and int(batch_images) < 1:
        raise ValueError(f"batch_images must be >= 1 or None, got {batch_images!r}")
    stage = device_stage or (GpuStage if batch_images is None else RaggedGpuStage)(watermark_data, block, alpha, preserve_ratio,
                                                                                 route=route)
    n_workers = workers or min(16, max(2, (len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 4)))
    with ThreadPoolExecutor(n_workers, thread_name_prefix="tmf-io") as pool:
        decoded: list[Future] = [pool.submit(_decode, s) for s in sources]
        encoded: list[Future] = []
        if batch_images is not None:  # the device stage takes groups of decoded images, in order
            for i0 in range(0, len(decoded), int(batch_images)):
                indices = list(range(i0, min(i0 + int(batch_images), len(decoded))))
                results = stage([decoded[i].result() for i in indices], indices)
                if len(results) != len(indices):
                    raise ValueError(f"the device stage returned {len(results)} results for {len(indices)} images")
                encoded.extend(pool.submit(_encode, pixels, wait) for pixels, wait in results)
            return [f.result() for f in encoded]
        for i, fut in enumerate(decoded):  # the device stage runs in order on this thread
            pixels, wait = stage(fut.result(), i) if per_image else stage(fut.result())
            encoded.append(pool.submit(_encode, pixels, wait))
        return [f.result() for f in encoded]
