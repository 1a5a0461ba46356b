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

``custom_settings`` may be a sequence of dicts, one per image (uploads of several sessions, each
with its own sliders): a group is then split by ``(block_size, svd_route)`` and each part is one
ragged call with its images' alphas (``embed_ragged(alpha=[...])``).

``extract_images`` is the extraction counterpart for a verifier that stores keys instead of
originals: decode on the worker threads, then per group of ``batch_images`` images of any
sizes one upload, one ``extract_keyed_ragged`` and one copy back (``KeyedExtractStage``).
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
    """One pipeline result: the watermarked RGB pixels and their PNG encoding; with
    ``embed_images(..., return_keys=True)`` also the extraction key of the original image
    (``watermarking.extraction_key``'s float32 array), else None."""

    pixels: np.ndarray
    png: bytes
    key: np.ndarray | None = None

    def image(self) -> Image.Image:
        return Image.fromarray(self.pixels, "RGB")


def _decode(src) -> np.ndarray:
    img = src if isinstance(src, Image.Image) else Image.open(io.BytesIO(src) if isinstance(src, (bytes, bytearray)) else src)
    return np.ascontiguousarray(np.asarray(img.convert("RGB"), dtype=np.uint8))


def _encode(pixels: np.ndarray, wait: Callable[[], None] | None, key: np.ndarray | None = None) -> Embedded:
    if wait is not None:
        wait()
    buf = io.BytesIO()
    Image.fromarray(pixels, "RGB").save(buf, format="PNG")  # embed_watermark_page.py:533-535
    return Embedded(pixels, buf.getvalue(), key)


class GpuStage:
    """Device stage: per image, pinned staging + side-stream H2D / embed / D2H.

    Returns (pixels, wait) where ``wait()`` blocks until the D2H copy landed.  The
    tile for an image size is prepared on the device once and reused.  ``watermark_data``
    may be a list or tuple of watermarks, one per image: the stage is then called as
    ``stage(rgb, i)`` and keeps its per-size tile cache per watermark.  With ``return_keys`` the
    embed is ``embed_with_key`` and the stage returns (pixels, wait, key), the key copied back
    with the pixels.  With per-image settings the stage of a block size and route is called with
    ``settings=`` the image's resolved settings and takes its alpha from there."""

    def __init__(self, watermark_data, block: int, alpha: float, preserve_ratio: bool, device=None, route: str = SVD_ROUTE,
                 return_keys: bool = False):
        import torch

        from . import batch

        self.torch, self.batch = torch, batch
        self.block, self.alpha, self.preserve_ratio = int(block), float(alpha), bool(preserve_ratio)
        self.route = route  # the drop-in's SVD route (constants.SVD_ROUTE, custom_settings["svd_route"])
        self.return_keys = bool(return_keys)
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

    def __call__(self, rgb: np.ndarray, index: int = 0, settings: dict | None = None):
        torch = self.torch
        alpha = self.alpha if settings is None else float(settings["alpha"])
        h, w = rgb.shape[:2]
        nbh, nbw = h // self.block, w // self.block
        if nbh == 0 or nbw == 0:
            raise ValueError("height and width must be > 0")  # PIL's resize raises in the reference
        host_in = torch.empty((1, h, w, 3), dtype=torch.uint8, pin_memory=True)
        host_in.numpy()[0] = rgb
        host_out = torch.empty((1, h, w, 3), dtype=torch.uint8, pin_memory=True)
        host_key = torch.empty((1, nbh, nbw), dtype=torch.float32, pin_memory=True) if self.return_keys else None
        tile = self._tile(nbh, nbw, index)
        with torch.cuda.stream(self.stream):
            dev_in = host_in.to(self.device, non_blocking=True)
            dev_key = None
            if self.return_keys:
                dev_out, dev_key = self.batch.embed_with_key(dev_in, tile, self.block, alpha, stream=self.stream, route=self.route)
                host_key.copy_(dev_key, non_blocking=True)
            else:
                dev_out = self.batch.embed_batch(dev_in, tile, self.block, alpha, stream=self.stream, route=self.route)
            host_out.copy_(dev_out, non_blocking=True)
            done = torch.cuda.Event()
            done.record(self.stream)
        # keep the device buffers alive until the copy has landed
        keep = (dev_in, dev_out, dev_key, host_in)

        def wait(_e=done, _k=keep):
            _e.synchronize()

        if self.return_keys:
            return host_out.numpy()[0], wait, host_key.numpy()[0]
        return host_out.numpy()[0], wait


class RaggedGpuStage(GpuStage):
    """Batched device stage (``embed_images(..., batch_images=K)``): a group of decoded images of
    any sizes is uploaded, one ``prepare_tiles_ragged`` makes the tiles the group needs and the
    cache does not hold, one ``embed_ragged`` embeds the whole group, and the results are copied
    back.

    Called as ``stage(rgbs, indices)`` with the group's pixel arrays and their positions in the
    input (the watermark of image ``i`` is watermark ``i`` when there is one per image); returns
    one ``(pixels, wait)`` per image, in the group's order -- with ``return_keys``, by one
    ``embed_with_key_ragged``, one ``(pixels, wait, key)`` per image.  With per-image settings
    ``settings=`` is the group's resolved settings, one dict per image, and the one ragged call
    takes their alphas."""

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

    def __call__(self, rgbs, indices, settings=None):
        torch = self.torch
        alpha = self.alpha if settings is None else [float(s["alpha"]) for s in settings]
        keys, host_in, host_out, host_key = [], [], [], []
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
            if self.return_keys:
                host_key.append(torch.empty((nbh, nbw), dtype=torch.float32, pin_memory=True))
        with torch.cuda.stream(self.stream):
            tiles = self._group_tiles(keys)
            dev_in = [h.to(self.device, non_blocking=True) for h in host_in]
            dev_key = []
            # the rank-1 routes have ragged calls of their own (batch.embed_ragged_rank1)
            rank1 = self.route in ("rank1", "rank1_reference")
            if self.return_keys:
                embed = self.batch.embed_with_key_ragged_rank1 if rank1 else self.batch.embed_with_key_ragged
                dev_out, dev_key = embed(dev_in, tiles, self.block, alpha, stream=self.stream, route=self.route)
            else:
                embed = self.batch.embed_ragged_rank1 if rank1 else self.batch.embed_ragged
                dev_out = embed(dev_in, tiles, self.block, alpha, stream=self.stream, route=self.route)
            for ho, do in zip(host_out + host_key, list(dev_out) + list(dev_key)):
                ho.copy_(do, non_blocking=True)
            done = torch.cuda.Event()
            done.record(self.stream)
        keep = (dev_in, dev_out, dev_key, host_in, tiles)  # alive until the copies have landed

        def wait(_e=done, _k=keep):
            _e.synchronize()

        if self.return_keys:
            return [(ho.numpy(), wait, hk.numpy()) for ho, hk in zip(host_out, host_key)]
        return [(ho.numpy(), wait) for ho in host_out]


def _check_key(i: int, key, h: int, w: int, block: int) -> None:
    """What watermarking.extract_watermark_keyed asks of a key, for image i of h x w pixels."""
    if not isinstance(key, np.ndarray) or key.dtype != np.float32:
        raise TypeError(f"keys[{i}] must be a float32 numpy array (extraction_key's result), got {getattr(key, 'dtype', type(key))}")
    if key.shape != (h // block, w // block):
        raise ValueError(f"keys[{i}] shape {key.shape} != ({h // block}, {w // block}) for a {w}x{h} image at block size {block}: "
                         "a key belongs to one block size and one image size")


class KeyedExtractStage:
    """Batched device stage of ``extract_images``: a group of decoded watermarked images of any
    sizes and their keys go up in one copy (a key that several images share goes up once), one
    ``extract_keyed_ragged`` extracts the whole group, and the tiles come back in one copy.

    Called as ``stage(rgbs, keys, indices)``; returns one ``(tile, wait)`` per image, in the
    group's order, where ``wait()`` blocks until the copy back has landed.  An image smaller
    than a block has no block: its tile is empty and it takes no part in the device call.  With
    per-image settings ``settings=`` is the group's resolved settings and the call takes their
    alphas."""

    def __init__(self, block: int, alpha: float, device=None, route: str = SVD_ROUTE):
        import torch

        from . import batch

        self.torch, self.batch = torch, batch
        self.block, self.alpha, self.route = int(block), float(alpha), route
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.stream = torch.cuda.Stream(device=self.device)

    def __call__(self, rgbs, keys, indices, settings=None):
        torch, b = self.torch, self.block
        live = [j for j, rgb in enumerate(rgbs) if rgb.shape[0] >= b and rgb.shape[1] >= b]
        tiles = [np.zeros((rgb.shape[0] // b, rgb.shape[1] // b), np.uint8) for rgb in rgbs]
        if not live:
            return [(t, None) for t in tiles]
        # one pinned buffer for the group's pixels and keys (16-byte aligned pieces), one for its tiles
        pieces, rgb_at, key_at, total = [], {}, {}, 0
        for j in live:
            for arr, at, name in ((rgbs[j], rgb_at, j), (keys[j], key_at, id(keys[j]))):
                if name not in at:
                    at[name] = total
                    pieces.append((total, arr))
                    total += (arr.nbytes + 15) & ~15
        host_in = torch.empty((total,), dtype=torch.uint8, pin_memory=True)
        flat = host_in.numpy()
        for off, arr in pieces:
            flat[off:off + arr.nbytes] = np.ascontiguousarray(arr).reshape(-1).view(np.uint8)
        out_at, out_total = [], 0
        for j in live:
            out_at.append(out_total)
            out_total += (tiles[j].size + 15) & ~15
        host_out = torch.empty((out_total,), dtype=torch.uint8, pin_memory=True)
        with torch.cuda.stream(self.stream):
            dev_in = host_in.to(self.device, non_blocking=True)
            dev_out = torch.empty((out_total,), dtype=torch.uint8, device=self.device)
            frames, dkeys, outs = [], [], []
            for j, o in zip(live, out_at):
                h, w = rgbs[j].shape[:2]
                nbh, nbw = h // b, w // b
                at = rgb_at[j]
                frames.append(dev_in[at:at + h * w * 3].view(h, w, 3))
                k0 = key_at[id(keys[j])]
                dkeys.append(dev_in[k0:k0 + 4 * nbh * nbw].view(torch.float32).view(nbh, nbw))
                outs.append(dev_out[o:o + nbh * nbw].view(nbh, nbw))
            # on a rank-1 route the keyed extract is the hybrid enclosure, as every single-size keyed call has it
            route = "hybrid" if self.route in ("rank1", "rank1_reference") else self.route
            alpha = self.alpha if settings is None else [float(settings[j]["alpha"]) for j in live]
            self.batch.extract_keyed_ragged(frames, dkeys, b, alpha, out=outs, stream=self.stream, route=route)
            host_out.copy_(dev_out, non_blocking=True)
            done = torch.cuda.Event()
            done.record(self.stream)
        keep = (dev_in, dev_out, host_in)  # alive until the copy back has landed

        def wait(_e=done, _k=keep):
            _e.synchronize()

        res = host_out.numpy()
        for j, o in zip(live, out_at):
            tiles[j] = res[o:o + tiles[j].size].reshape(tiles[j].shape)
        return [(t, wait if j in live else None) for j, t in enumerate(tiles)]


def _resolved(settings) -> dict:
    """One image's settings with the defaults filled in, as the drop-ins read them."""
    s = settings or {}
    return {"block_size": int(s.get("block_size", BLOCK_SIZE)), "alpha": float(s.get("alpha", ALPHA)),
            "svd_route": s.get("svd_route") or os.environ.get("TMFWM_SVD_ROUTE") or SVD_ROUTE}  # as watermarking._route


def _per_image_settings(custom_settings, n: int) -> list:
    if len(custom_settings) != n:
        raise ValueError(f"{len(custom_settings)} settings for {n} images: custom_settings is one dict, or one per image")
    return [_resolved(s) for s in custom_settings]


def _parts(indices, resolved) -> dict:
    """A group's positions by (block_size, svd_route), in order of first appearance: one ragged
    call takes one block size and one route, and any alphas."""
    parts: dict = {}
    for j, i in enumerate(indices):
        parts.setdefault((resolved[i]["block_size"], resolved[i]["svd_route"]), []).append(j)
    return parts


def _staged_parts(indices, resolved, call) -> list:
    """The group's results in its own order, from one call(block, route, positions, settings) per part."""
    results = [None] * len(indices)
    for (block, route), js in _parts(indices, resolved).items():
        part = call(block, route, js, [resolved[indices[j]] for j in js])
        if len(part) != len(js):
            raise ValueError(f"the device stage returned {len(part)} results for {len(js)} images")
        for j, r in zip(js, part):
            results[j] = r
    return results


def extract_images(images: Iterable, keys: Sequence, custom_settings: dict | None = None, batch_images: int = 16,
                   workers: int | None = None, device_stage: Callable | None = None):
    """The extraction counterpart of ``embed_images`` for a verifier that stores keys
    (``watermarking.extraction_key``) instead of originals: yields, in input order, the
    (W/b) x (H/b) mode-"L" extracted watermark of every watermarked image (bytes, file object or
    PIL image) against ``keys[i]``, pixel for pixel ``extract_watermark_keyed(images[i], keys[i],
    custom_settings)``.  The same key array may stand for several images.

    Images are decoded on worker threads and taken ``batch_images`` at a time, of any sizes:
    each group is one upload, one ``extract_keyed_ragged`` and one copy back
    (``KeyedExtractStage``; a custom ``device_stage`` is called as ``stage(rgbs, keys, indices)``
    and returns one ``(tile, wait)`` per image).  A key that is not float32 (TypeError) or whose
    shape does not fit its image (ValueError) raises before any device work for its group.
    Decoding the tiles' QR content stays with the caller (``qrcode_generator.qrcode_to_text``).

    ``custom_settings`` may be a list or tuple of dicts, one per image (another length is a
    ValueError): result i is then ``extract_watermark_keyed(images[i], keys[i], custom_settings[i])``.
    Each group is split by ``(block_size, svd_route)`` and each part is one ``extract_keyed_ragged``
    with its images' alphas; a custom ``device_stage`` is called once per part as
    ``stage(rgbs, keys, indices, settings=[...])`` with the part's resolved settings."""
    per_settings = isinstance(custom_settings, (list, tuple))
    settings = {} if per_settings else custom_settings or {}
    block = int(settings.get("block_size", BLOCK_SIZE))
    alpha = float(settings.get("alpha", ALPHA))
    route = settings.get("svd_route") or os.environ.get("TMFWM_SVD_ROUTE") or SVD_ROUTE  # as watermarking._route
    sources: Sequence = list(images)
    keys = list(keys)
    if len(keys) != len(sources):
        raise ValueError(f"{len(keys)} keys for {len(sources)} images")
    resolved = _per_image_settings(custom_settings, len(sources)) if per_settings else None
    if batch_images is None or int(batch_images) < 1:
        raise ValueError(f"batch_images must be >= 1, got {batch_images!r}")
    if per_settings:
        for r in resolved:
            if r["block_size"] <= 0:
                raise ValueError(f"block_size must be positive, got {r['block_size']}")
        stages: dict = {}  # one default stage per (block size, route)

        def stage(rgbs, group_keys, indices):
            def call(b, rt, js, part_settings):
                if device_stage is None and (b, rt) not in stages:
                    stages[(b, rt)] = KeyedExtractStage(b, ALPHA, route=rt)
                return (device_stage or stages[(b, rt)])([rgbs[j] for j in js], [group_keys[j] for j in js], [indices[j] for j in js],
                                                         settings=part_settings)

            return _staged_parts(indices, resolved, call)
    else:
        if block <= 0:
            raise ValueError(f"block_size must be positive, got {block}")
        stage = device_stage or KeyedExtractStage(block, alpha, route=route)
    n_workers = workers or min(16, max(2, (len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 4)))

    def finish(results):
        for tile, wait in results:
            if wait is not None:
                wait()
            yield Image.fromarray(tile)

    def run():
        with ThreadPoolExecutor(n_workers, thread_name_prefix="tmf-io") as pool:
            decoded: list[Future] = [pool.submit(_decode, s) for s in sources]
            pending = None  # the group on the device while the next one is checked and uploaded
            for i0 in range(0, len(decoded), int(batch_images)):
                indices = list(range(i0, min(i0 + int(batch_images), len(decoded))))
                rgbs = [decoded[i].result() for i in indices]
                for i, rgb in zip(indices, rgbs):
                    _check_key(i, keys[i], rgb.shape[0], rgb.shape[1], resolved[i]["block_size"] if per_settings else block)
                results = stage(rgbs, [keys[i] for i in indices], indices)
                if len(results) != len(indices):
                    raise ValueError(f"the device stage returned {len(results)} results for {len(indices)} images")
                if pending is not None:
                    yield from finish(pending)
                pending = results
            if pending is not None:
                yield from finish(pending)

    return run()


def embed_images(images: Iterable, watermark_data, preserve_ratio: bool = True, custom_settings: dict | None = None,
                 workers: int | None = None, device_stage: Callable | None = None,
                 batch_images: int | None = None, return_keys: bool = False) -> list[Embedded]:
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
    which ``None`` keeps.

    ``return_keys=True`` is the enrolment side of keyed extraction: every ``Embedded`` also carries
    ``key``, bit for bit ``watermarking.extraction_key(image, custom_settings)`` of the original
    image, out of the same device call as the pixels (``embed_with_key`` /
    ``embed_with_key_ragged``) -- what ``extract_images`` takes with the watermarked images.  A
    custom ``device_stage`` then returns ``(pixels, wait, key)`` per image.

    ``custom_settings`` may be a list or tuple of dicts, one per image (another length is a
    ValueError): result i is then ``embed_watermark(images[i], watermark_i, preserve_ratio,
    custom_settings[i])``.  With ``batch_images=K`` each group of K images is split by
    ``(block_size, svd_route)`` and each part goes through one ragged call with its images'
    alphas; without it the per-image stage takes each image's settings.  A custom ``device_stage``
    additionally receives ``settings=``: the part's resolved settings, one dict per image (the
    image's dict on the per-image path).  A single dict behaves as it always has."""
    if isinstance(custom_settings, (list, tuple)):
        return _embed_images_per_settings(images, watermark_data, preserve_ratio, custom_settings, workers, device_stage,
                                          batch_images, return_keys)
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
                                                                                 route=route, **({"return_keys": True} if return_keys else {}))
    arity = 3 if return_keys else 2

    def checked(result):
        if len(result) != arity:
            raise ValueError(f"the device stage returned {len(result)} values per image, {arity} expected"
                             + (" (pixels, wait, key)" if return_keys else ""))
        return result

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
                encoded.extend(pool.submit(_encode, *checked(r)) for r in results)
            return [f.result() for f in encoded]
        for i, fut in enumerate(decoded):  # the device stage runs in order on this thread
            encoded.append(pool.submit(_encode, *checked(stage(fut.result(), i) if per_image else stage(fut.result()))))
        return [f.result() for f in encoded]


def _embed_images_per_settings(images, watermark_data, preserve_ratio, custom_settings, workers, device_stage, batch_images,
                               return_keys) -> list[Embedded]:
    """embed_images with one settings dict per image."""
    sources: Sequence = list(images)
    per_image = isinstance(watermark_data, (list, tuple))
    if per_image and len(watermark_data) != len(sources):
        raise ValueError(f"{len(watermark_data)} watermarks for {len(sources)} images")
    resolved = _per_image_settings(custom_settings, len(sources))
    if batch_images is not None and int(batch_images) < 1:
        raise ValueError(f"batch_images must be >= 1 or None, got {batch_images!r}")
    stages: dict = {}  # one default stage per (block size, route)

    def stage_of(block, route):
        if device_stage is not None:
            return device_stage
        if (block, route) not in stages:
            stages[(block, route)] = (GpuStage if batch_images is None else RaggedGpuStage)(
                watermark_data, block, ALPHA, preserve_ratio, route=route, **({"return_keys": True} if return_keys else {}))
        return stages[(block, route)]

    arity = 3 if return_keys else 2

    def checked(result):
        if len(result) != arity:
            raise ValueError(f"the device stage returned {len(result)} values per image, {arity} expected"
                             + (" (pixels, wait, key)" if return_keys else ""))
        return result

    n_workers = workers or min(16, max(2, (len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 4)))
    with ThreadPoolExecutor(n_workers, thread_name_prefix="tmf-io") as pool:
        decoded: list[Future] = [pool.submit(_decode, s) for s in sources]
        encoded: list[Future] = []
        if batch_images is not None:
            for i0 in range(0, len(decoded), int(batch_images)):
                indices = list(range(i0, min(i0 + int(batch_images), len(decoded))))
                rgbs = [decoded[i].result() for i in indices]

                def call(block, route, js, part_settings):
                    return stage_of(block, route)([rgbs[j] for j in js], [indices[j] for j in js], settings=part_settings)

                encoded.extend(pool.submit(_encode, *checked(r)) for r in _staged_parts(indices, resolved, call))
            return [f.result() for f in encoded]
        for i, fut in enumerate(decoded):
            stage = stage_of(resolved[i]["block_size"], resolved[i]["svd_route"])
            res = stage(fut.result(), i, settings=resolved[i]) if per_image else stage(fut.result(), settings=resolved[i])
            encoded.append(pool.submit(_encode, *checked(res)))
        return [f.result() for f in encoded]
