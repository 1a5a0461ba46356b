"""Device-resident batch API: frames already in HBM (torch tensors on a ROCm GPU).

This is the path the benchmark and multi-GPU driver use: a batch of N frames
(N, H, W, 3) uint8 on ``cuda:k`` is embedded / extracted by ONE kernel launch
each, enqueued on the caller's current torch stream.  torch provides device
memory and streams only; the arithmetic is libtmfwm.so's HIP kernels.
"""
from __future__ import annotations

import torch

from . import _lib
from .constants import SUPPORTED_BLOCK_SIZES

SEED_COVER = 0x5EED0001
SEED_WATERMARK = 0x5EED0002


def _stream(stream) -> int:
    s = stream if stream is not None else torch.cuda.current_stream()
    return int(s.cuda_stream)


def _check_frames(t: torch.Tensor, name: str, px=(3,)) -> None:
    """px: the pixel sizes the call takes -- (3,), or (3, 4) for the keyed calls, which also read
    R G B pad frames (the pad byte is ignored)."""
    if not t.is_cuda:
        raise ValueError(f"{name} must be a GPU tensor")
    if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[-1] not in px:
        want = " or ".join(f"(N, H, W, {p})" for p in px)
        raise ValueError(f"{name} must be {want} uint8, got {tuple(t.shape)} {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def _count_ptr(stats):
    import ctypes

    if stats is None:
        return None, None
    c = ctypes.c_int64(0)
    return c, ctypes.addressof(c)


def embed_list_pass(block: int) -> bool:
    """Whether embed at this block size runs a list pass after its strip pass."""
    return bool(_lib.load().tmfwm_embed_list_pass(int(block)))


def embed_batch(frames: torch.Tensor, wm_tile: torch.Tensor, block: int = 8, alpha: float = 0.1,
                out: torch.Tensor | None = None, stream=None, stats: dict | None = None,
                route: str = "hybrid") -> torch.Tensor:
    """Embed one watermark tile into every frame (watermarking.py:135 per frame), or one tile
    per frame: wm_tile is (H/b, W/b), shared, or (N, H/b, W/b), frame f getting wm_tile[f].
    stats (optional dict) receives "lapack_blocks": the blocks redone on the dgesdd route;
    asking for it synchronises the stream.  route: "hybrid" (Jacobi + the dgesdd route for
    the flagged blocks, the throughput route) or "reference" (the dgesdd route for every
    block: np.linalg.svd's arithmetic by construction)."""
    _check_frames(frames, "frames")
    n, h, w, _ = frames.shape
    if block not in SUPPORTED_BLOCK_SIZES:
        raise NotImplementedError(f"block {block}")
    nbh, nbw = h // block, w // block
    if tuple(wm_tile.shape) not in ((nbh, nbw), (n, nbh, nbw)) or wm_tile.dtype != torch.uint8 or not wm_tile.is_cuda:
        raise ValueError(f"wm_tile must be ({nbh}, {nbw}) or ({n}, {nbh}, {nbw}) uint8 on the GPU, got {tuple(wm_tile.shape)}")
    wm_tile = wm_tile.contiguous()
    if out is None:
        out = torch.empty_like(frames)
    else:
        _check_frames(out, "out")
        if out.shape != frames.shape:
            raise ValueError("out shape mismatch")
    cnt, ptr = _count_ptr(stats)
    with torch.cuda.device(frames.device):
        L = _lib.load()
        if wm_tile.dim() == 2:
            rc = L.tmfwm_embed_route(frames.data_ptr(), n, h, w, h * w * 3, wm_tile.data_ptr(), block, float(alpha),
                                     out.data_ptr(), _lib.MEM_DEVICE, _stream(stream), _lib.route_code(route), ptr)
        else:  # one tile per frame, nbh * nbw bytes apart
            rc = L.tmfwm_embed_tiles(frames.data_ptr(), _lib.PIX_RGB, h * w * 3, n, h, w, wm_tile.data_ptr(), nbh * nbw, block,
                                     float(alpha), out.data_ptr(), _lib.PIX_RGB, h * w * 3, _lib.MEM_DEVICE, _stream(stream),
                                     _lib.route_code(route), ptr)
        _lib.check(rc, "embed_batch")
    if stats is not None:
        stats["lapack_blocks"] = int(cnt.value)
        stats["list_pass_blocks"] = int(L.tmfwm_last_list_pass_blocks())
    return out


def extract_batch(wframes: torch.Tensor, oframes: torch.Tensor, block: int = 8, alpha: float = 0.1,
                  out: torch.Tensor | None = None, stream=None, stats: dict | None = None,
                  route: str = "hybrid") -> torch.Tensor:
    """Extract the watermark tile of every frame pair (watermarking.py:224 per pair).
    stats (optional dict) receives "lapack_blocks" (synchronises the stream); route as
    embed_batch's."""
    _check_frames(wframes, "wframes")
    _check_frames(oframes, "oframes")
    if wframes.shape != oframes.shape:
        raise ValueError("watermarked / original batch shapes differ")
    n, h, w, _ = wframes.shape
    if block not in SUPPORTED_BLOCK_SIZES:
        raise NotImplementedError(f"block {block}")
    if out is None:
        out = torch.empty((n, h // block, w // block), dtype=torch.uint8, device=wframes.device)
    cnt, ptr = _count_ptr(stats)
    with torch.cuda.device(wframes.device):
        L = _lib.load()
        _lib.check(L.tmfwm_extract_route(wframes.data_ptr(), oframes.data_ptr(), n, h, w, h * w * 3, block, float(alpha),
                                         out.data_ptr(), _lib.MEM_DEVICE, _stream(stream), _lib.route_code(route), ptr),
                   "extract_batch")
    if stats is not None:
        stats["lapack_blocks"] = int(cnt.value)
        stats["list_pass_blocks"] = int(L.tmfwm_last_list_pass_blocks())
    return out


def sigma1_map(frames: torch.Tensor, block: int = 8, out: torch.Tensor | None = None, stream=None,
               stats: dict | None = None, route: str = "hybrid") -> torch.Tensor:
    """The extraction key of every frame: float32 (N, H//b, W//b), f32(sigma_1) of each block's
    DCT -- all that extract uses of an original image.  The key is the same bit
    for bit on every route.  frames is (N, H, W, 3), or (N, H, W, 4) R G B pad, which is read
    in place and gives the key of its R, G, B values.  stats and route as extract_batch's."""
    _check_frames(frames, "frames", (3, 4))
    n, h, w, px = frames.shape
    if block not in SUPPORTED_BLOCK_SIZES:
        raise NotImplementedError(f"block {block}")
    shape = (n, h // block, w // block)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=frames.device)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or out.device != frames.device or not out.is_contiguous():
        raise ValueError(f"out must be {shape} float32, contiguous, on the frames' device")
    cnt, ptr = _count_ptr(stats)
    with torch.cuda.device(frames.device):
        L = _lib.load()
        _lib.check(L.tmfwm_sigma1_map_px(frames.data_ptr(), px, h * w * px, n, h, w, block, out.data_ptr(), _lib.MEM_DEVICE,
                                         _stream(stream), _lib.route_code(route), ptr), "sigma1_map")
    if stats is not None:
        stats["lapack_blocks"] = int(cnt.value)
        stats["list_pass_blocks"] = int(L.tmfwm_last_list_pass_blocks())
    return out


def extract_keyed(wframes: torch.Tensor, key: torch.Tensor, block: int = 8, alpha: float = 0.1,
                  out: torch.Tensor | None = None, stream=None, stats: dict | None = None,
                  route: str = "hybrid") -> torch.Tensor:
    """extract_batch without the original frames: key is sigma1_map of the original(s), (H//b, W//b)
    shared by every frame (one original, many watermarked copies) or (N, H//b, W//b).  The
    bytes are extract_batch's.  A key belongs to one block size and one image size.  wframes is
    (N, H, W, 3), or (N, H, W, 4) R G B pad, read in place.  stats and route as extract_batch's."""
    _check_frames(wframes, "wframes", (3, 4))
    n, h, w, px = wframes.shape
    if block not in SUPPORTED_BLOCK_SIZES:
        raise NotImplementedError(f"block {block}")
    nbh, nbw = h // block, w // block
    if not isinstance(key, torch.Tensor) or key.dtype != torch.float32:
        raise TypeError("key must be a float32 tensor")
    if tuple(key.shape) not in ((nbh, nbw), (n, nbh, nbw)):
        raise ValueError(f"key must be ({nbh}, {nbw}) or ({n}, {nbh}, {nbw}) for block {block} and {w}x{h} frames, "
                         f"got {tuple(key.shape)}: a key belongs to one block size and one image size")
    if key.device != wframes.device or not key.is_contiguous():
        raise ValueError("key must be contiguous and on the frames' device")
    if out is None:
        out = torch.empty((n, nbh, nbw), dtype=torch.uint8, device=wframes.device)
    elif tuple(out.shape) != (n, nbh, nbw) or out.dtype != torch.uint8 or out.device != wframes.device or not out.is_contiguous():
        raise ValueError(f"out must be ({n}, {nbh}, {nbw}) uint8, contiguous, on the frames' device")
    cnt, ptr = _count_ptr(stats)
    with torch.cuda.device(wframes.device):
        L = _lib.load()
        _lib.check(L.tmfwm_extract_keyed_px(wframes.data_ptr(), px, h * w * px, n, h, w, key.data_ptr(),
                                            0 if key.dim() == 2 else nbh * nbw * 4, block, float(alpha), out.data_ptr(),
                                            _lib.MEM_DEVICE, _stream(stream), _lib.route_code(route), ptr), "extract_keyed")
    if stats is not None:
        stats["lapack_blocks"] = int(cnt.value)
        stats["list_pass_blocks"] = int(L.tmfwm_last_list_pass_blocks())
    return out


def embed_with_key(frames: torch.Tensor, wm_tile: torch.Tensor, block: int = 8, alpha: float = 0.1,
                   out: torch.Tensor | None = None, key_out: torch.Tensor | None = None, stream=None,
                   stats: dict | None = None, route: str = "hybrid"):
    """embed_batch that also returns the extraction key of the ORIGINAL frames, in one call
    (tmfwm_embed_key): (out, key), out the bytes of embed_batch(frames, wm_tile, ...), key the
    float32 (N, H//b, W//b) bits of sigma1_map(frames, block) -- what extract_keyed takes with
    `out`.  On the hybrid and reference routes the key comes out of the embed passes themselves
    (DESIGN.md 5); on the rank-1 routes the call runs the map's passes after the embed's.
    wm_tile, stats and route as embed_batch's; "lapack_blocks" counts a block whose key the
    dgesdd route had to decide as well.  frames may be (N, H, W, 4) R G B pad: the output then is
    4-byte as well, pad 255 (or whatever layout `out` has), converted on the device."""
    _check_frames(frames, "frames", (3, 4))
    n, h, w, px = frames.shape
    if block not in SUPPORTED_BLOCK_SIZES:
        raise NotImplementedError(f"block {block}")
    nbh, nbw = h // block, w // block
    if tuple(wm_tile.shape) not in ((nbh, nbw), (n, nbh, nbw)) or wm_tile.dtype != torch.uint8 or not wm_tile.is_cuda:
        raise ValueError(f"wm_tile must be ({nbh}, {nbw}) or ({n}, {nbh}, {nbw}) uint8 on the GPU, got {tuple(wm_tile.shape)}")
    wm_tile = wm_tile.contiguous()
    if out is None:
        out = torch.empty_like(frames)
    else:
        _check_frames(out, "out", (3, 4))
        if out.shape[:3] != frames.shape[:3]:
            raise ValueError("out shape mismatch")
    opx = out.shape[-1]
    shape = (n, nbh, nbw)
    if key_out is None:
        key_out = torch.empty(shape, dtype=torch.float32, device=frames.device)
    elif (not isinstance(key_out, torch.Tensor) or tuple(key_out.shape) != shape or key_out.dtype != torch.float32
          or key_out.device != frames.device or not key_out.is_contiguous()):
        raise ValueError(f"key_out must be {shape} float32, contiguous, on the frames' device")
    cnt, ptr = _count_ptr(stats)
    with torch.cuda.device(frames.device):
        L = _lib.load()
        _lib.check(L.tmfwm_embed_key_px(frames.data_ptr(), px, h * w * px, n, h, w, wm_tile.data_ptr(),
                                        0 if wm_tile.dim() == 2 else nbh * nbw, block, float(alpha), out.data_ptr(), opx, h * w * opx,
                                        key_out.data_ptr(), nbh * nbw * 4, _lib.MEM_DEVICE, _stream(stream), _lib.route_code(route),
                                        ptr), "embed_with_key")
    if stats is not None:
        stats["lapack_blocks"] = int(cnt.value)
        stats["list_pass_blocks"] = int(L.tmfwm_last_list_pass_blocks())
    return out, key_out


def _check_ragged(frames, name: str, device=None, px=(3,)):
    """A sequence of (H_i, W_i, 3) uint8 contiguous GPU tensors on one device -> (list, device).
    px = (3, 4): the keyed calls, which take (H_i, W_i, 4) R G B pad frames as well -- one layout per
    call, looked at before anything else about the tensors."""
    frames = list(frames)
    if len(px) > 1:
        sizes = {int(t.shape[-1]) for t in frames if isinstance(t, torch.Tensor) and t.dim() == 3 and t.shape[-1] in px}
        if len(sizes) > 1:
            raise ValueError(f"{name} mixes 3- and 4-byte pixels: one pixel layout per call")
    for i, t in enumerate(frames):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError(f"{name}[{i}] must be a GPU tensor")
        if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[-1] not in px:
            want = " or ".join(f"(H, W, {p})" for p in px)
            raise ValueError(f"{name}[{i}] must be {want} uint8, got {tuple(t.shape)} {t.dtype}")
        if not t.is_contiguous():
            raise ValueError(f"{name}[{i}] must be contiguous")
        device = t.device if device is None else device
        if t.device != device:
            raise ValueError(f"{name}[{i}] is on {t.device}, the call's other tensors on {device}")
    return frames, device


def _ragged_views(sizes, shape_of, device) -> list:
    """One uint8 device allocation cut into per-frame views (each 16-byte aligned)."""
    offs, total = [], 0
    for s in sizes:
        offs.append(total)
        total += (s + 15) & ~15
    buf = torch.empty((total,), dtype=torch.uint8, device=device)
    return [buf[o:o + s].view(shape_of(i)) for i, (o, s) in enumerate(zip(offs, sizes))]


def _ragged_route(route) -> int:
    code = _lib.route_code(route)
    if code in (_lib.ROUTE_RANK1, _lib.ROUTE_RANK1_REFERENCE):
        raise NotImplementedError("the ragged calls do not take the rank-1 routes yet")
    return code


def _ragged_alphas(alpha, n: int, what: str = "frames"):
    """The alpha of a ragged call: a number -- None, the uniform entry takes float(alpha) -- or a
    sequence of one alpha per frame -- a C array of n doubles for the *_ragged_alphas entry.  A
    sequence of another length is a ValueError, raised before anything about the tensors or the
    device is looked at."""
    import ctypes
    import numbers

    # a number in any dress (a Python or numpy scalar, a 0-d array or tensor) is the uniform call's
    if isinstance(alpha, numbers.Real) or getattr(alpha, "ndim", None) == 0:
        return None
    try:
        vals = [float(a) for a in alpha]  # a list, tuple, 1-d array or tensor, or any other iterable
    except TypeError:
        raise TypeError(f"alpha must be a number or a sequence of one number per frame, got {type(alpha).__name__}") from None
    if len(vals) != n:
        raise ValueError(f"{len(vals)} alphas for {n} {what}: alpha is one number, or one per frame")
    return (ctypes.c_double * max(n, 1))(*vals)


def _embed_ragged_args(frames, tiles, block, route, out, rank1_routes: bool = False):
    """embed_ragged's checks and output views: (frames, tiles, out, device, route code)."""
    if block not in SUPPORTED_BLOCK_SIZES:
        raise NotImplementedError(f"block {block}")
    code = _lib.route_code(route) if rank1_routes else _ragged_route(route)
    frames, dev = _check_ragged(frames, "frames")
    tiles = list(tiles)
    if len(tiles) != len(frames):
        raise ValueError(f"{len(tiles)} tiles for {len(frames)} frames")
    for i, (f, t) in enumerate(zip(frames, tiles)):
        want = (f.shape[0] // block, f.shape[1] // block)
        if (not isinstance(t, torch.Tensor) or tuple(t.shape) != want or t.dtype != torch.uint8 or t.device != dev
                or not t.is_contiguous()):
            raise ValueError(f"tiles[{i}] must be a contiguous {want} uint8 tensor on {dev}")
    if out is None:
        out = _ragged_views([f.numel() for f in frames], lambda i: frames[i].shape, dev) if frames else []
    else:
        out, _ = _check_ragged(out, "out", dev)
        if len(out) != len(frames) or any(o.shape != f.shape for o, f in zip(out, frames)):
            raise ValueError("out must hold one tensor per frame, shaped like it")
    return frames, tiles, out, dev, code


def embed_ragged_rank1(frames, tiles, block: int = 8, alpha: float = 0.1, out=None, stream=None, stats: dict | None = None,
                       route: str = "rank1") -> list:
    """embed_ragged on every route (tmfwm_embed_ragged_rank1): "rank1" and "rank1_reference" run the
    rank-1 pre-pass over all the frames' blocks in one launch, and what it leaves goes to one list
    pass on the hybrid route ("rank1") or straight to the dgesdd route ("rank1_reference");
    "hybrid" and "reference" are embed_ragged itself.  Arguments, checks and the return value are
    embed_ragged's; output i is the bytes of embed_batch(frames[i][None], tiles[i], ..., route=route)[0].
    stats["list_pass_blocks"] is what the pre-pass left to the list pass on "rank1"."""
    import ctypes

    frames = list(frames)
    alphas = _ragged_alphas(alpha, len(frames))
    frames, tiles, out, dev, code = _embed_ragged_args(frames, tiles, block, route, out, rank1_routes=True)
    desc = (_lib.EmbedFrame * max(len(frames), 1))()
    for i, (f, t, o) in enumerate(zip(frames, tiles, out)):
        desc[i] = _lib.EmbedFrame(f.data_ptr(), o.data_ptr(), t.data_ptr(), f.shape[0], f.shape[1])
    cnt, ptr = _count_ptr(stats)
    L = _lib.load()
    if frames:
        with torch.cuda.device(dev):
            if alphas is None:
                rc = L.tmfwm_embed_ragged_rank1(ctypes.addressof(desc), len(frames), block, float(alpha), _lib.MEM_DEVICE,
                                                _stream(stream), code, ptr)
            else:
                rc = L.tmfwm_embed_ragged_alphas(ctypes.addressof(desc), ctypes.addressof(alphas), len(frames), block,
                                                 _lib.MEM_DEVICE, _stream(stream), code, ptr)
            _lib.check(rc, "embed_ragged_rank1")
    if stats is not None:
        stats["lapack_blocks"] = int(cnt.value)
        stats["list_pass_blocks"] = int(L.tmfwm_last_list_pass_blocks()) if frames else 0
    return list(out)


def embed_ragged(frames, tiles, block: int = 8, alpha: float = 0.1, out=None, stream=None, stats: dict | None = None,
                 route: str = "hybrid") -> list:
    """Embed frames of mixed sizes, each with its own tile, by one set of launches
    (tmfwm_embed_ragged): frames[i] is (H_i, W_i, 3) uint8, tiles[i] (H_i // block, W_i // block)
    uint8, all contiguous on one GPU.  Returns the outputs as per-frame views of one device
    allocation (or `out`, a sequence of tensors shaped like the frames); output i is the bytes
    of embed_batch(frames[i][None], tiles[i], ...)[0].  A frame smaller than a block gets its
    colour round trip.  stats and route ("hybrid" / "reference") as embed_batch's; no list pass
    runs, so "list_pass_blocks" is 0.  alpha is one number, or a sequence of len(frames) numbers,
    one per frame (tmfwm_embed_ragged_alphas; here and in the other ragged calls that take an
    alpha): output i is then embed_batch's at alpha[i], and a sequence of another length is a
    ValueError before any device work."""
    import ctypes

    frames = list(frames)
    alphas = _ragged_alphas(alpha, len(frames))
    frames, tiles, out, dev, code = _embed_ragged_args(frames, tiles, block, route, out)
    desc = (_lib.EmbedFrame * max(len(frames), 1))()
    for i, (f, t, o) in enumerate(zip(frames, tiles, out)):
        desc[i] = _lib.EmbedFrame(f.data_ptr(), o.data_ptr(), t.data_ptr(), f.shape[0], f.shape[1])
    cnt, ptr = _count_ptr(stats)
    L = _lib.load()
    if frames:
        with torch.cuda.device(dev):
            if alphas is None:
                rc = L.tmfwm_embed_ragged(ctypes.addressof(desc), len(frames), block, float(alpha), _lib.MEM_DEVICE,
                                          _stream(stream), code, ptr)
            else:
                rc = L.tmfwm_embed_ragged_alphas(ctypes.addressof(desc), ctypes.addressof(alphas), len(frames), block,
                                                 _lib.MEM_DEVICE, _stream(stream), code, ptr)
            _lib.check(rc, "embed_ragged")
    if stats is not None:
        stats["lapack_blocks"] = int(cnt.value)
        stats["list_pass_blocks"] = int(L.tmfwm_last_list_pass_blocks()) if frames else 0
    return list(out)


def extract_ragged(wframes, oframes, block: int = 8, alpha: float = 0.1, out=None, stream=None, stats: dict | None = None,
                   route: str = "hybrid") -> list:
    """Extract the tiles of frame pairs of mixed sizes by one set of launches
    (tmfwm_extract_ragged): wframes[i] and oframes[i] are (H_i, W_i, 3) uint8 of one shape.
    Returns per-frame (H_i // block, W_i // block) tiles, views of one device allocation (or
    `out`); tile i is the bytes of extract_batch(wframes[i][None], oframes[i][None], ...)[0]."""
    import ctypes

    wframes = list(wframes)
    alphas = _ragged_alphas(alpha, len(wframes))
    if block not in SUPPORTED_BLOCK_SIZES:
        raise NotImplementedError(f"block {block}")
    code = _ragged_route(route)
    wframes, dev = _check_ragged(wframes, "wframes")
    oframes, _ = _check_ragged(oframes, "oframes", dev)
    if len(wframes) != len(oframes):
        raise ValueError(f"{len(wframes)} watermarked frames for {len(oframes)} originals")
    for i, (w, o) in enumerate(zip(wframes, oframes)):
        if w.shape != o.shape:
            raise ValueError(f"wframes[{i}] / oframes[{i}] shapes differ")
    shapes = [(w.shape[0] // block, w.shape[1] // block) for w in wframes]
    if out is None:
        out = _ragged_views([a * b for a, b in shapes], lambda i: shapes[i], dev) if wframes else []
    else:
        out = list(out)
        if len(out) != len(wframes):
            raise ValueError("out must hold one tile per frame")
        for i, t in enumerate(out):
            if (not isinstance(t, torch.Tensor) or tuple(t.shape) != shapes[i] or t.dtype != torch.uint8 or t.device != dev
                    or not t.is_contiguous()):
                raise ValueError(f"out[{i}] must be a contiguous {shapes[i]} uint8 tensor on {dev}")
    desc = (_lib.ExtractFrame * max(len(wframes), 1))()
    for i, (w, o, t) in enumerate(zip(wframes, oframes, out)):
        desc[i] = _lib.ExtractFrame(w.data_ptr(), o.data_ptr(), t.data_ptr(), w.shape[0], w.shape[1])
    cnt, ptr = _count_ptr(stats)
    L = _lib.load()
    if wframes:
        with torch.cuda.device(dev):
            if alphas is None:
                rc = L.tmfwm_extract_ragged(ctypes.addressof(desc), len(wframes), block, float(alpha), _lib.MEM_DEVICE,
                                            _stream(stream), code, ptr)
            else:
                rc = L.tmfwm_extract_ragged_alphas(ctypes.addressof(desc), ctypes.addressof(alphas), len(wframes), block,
                                                   _lib.MEM_DEVICE, _stream(stream), code, ptr)
            _lib.check(rc, "extract_ragged")
    if stats is not None:
        stats["lapack_blocks"] = int(cnt.value)
        stats["list_pass_blocks"] = int(L.tmfwm_last_list_pass_blocks()) if wframes else 0
    return list(out)


def _check_ragged_out(out, shapes, dtype, dev, what: str) -> list:
    """The caller's outputs of a ragged keyed call: one contiguous tensor of shapes[i] per frame."""
    out = list(out)
    if len(out) != len(shapes):
        raise ValueError(f"out must hold one {what} per frame")
    for i, t in enumerate(out):
        if (not isinstance(t, torch.Tensor) or tuple(t.shape) != shapes[i] or t.dtype != dtype or t.device != dev
                or not t.is_contiguous()):
            raise ValueError(f"out[{i}] must be a contiguous {shapes[i]} {dtype} tensor on {dev}")
    return out


def sigma1_map_ragged(frames, block: int = 8, out=None, stream=None, stats: dict | None = None, route: str = "hybrid") -> list:
    """The extraction keys of frames of mixed sizes by one set of launches
    (tmfwm_sigma1_map_ragged_px): frames[i] is (H_i, W_i, 3) uint8 -- or every frame (H_i, W_i, 4)
    R G B pad, read in place; a mix is a ValueError -- contiguous, all on one GPU.
    Returns per-frame float32 (H_i // block, W_i // block) keys, views of one device allocation
    (or `out`, a sequence of such tensors); key i is sigma1_map(frames[i][None], ...)[0] bit for
    bit.  stats and route ("hybrid" / "reference") as sigma1_map's; no list pass runs, so
    "list_pass_blocks" is 0."""
    import ctypes

    if block not in SUPPORTED_BLOCK_SIZES:
        raise NotImplementedError(f"block {block}")
    code = _ragged_route(route)
    frames, dev = _check_ragged(frames, "frames", px=(3, 4))
    px = int(frames[0].shape[-1]) if frames else 3
    shapes = [(f.shape[0] // block, f.shape[1] // block) for f in frames]
    if out is None:  # float32 views of the one uint8 allocation: its pieces start on 16-byte boundaries
        out = [v.view(torch.float32).view(shapes[i]) for i, v in enumerate(
            _ragged_views([4 * a * b for a, b in shapes], lambda i: (4 * shapes[i][0] * shapes[i][1],), dev))] if frames else []
    else:
        out = _check_ragged_out(out, shapes, torch.float32, dev, "key")
    desc = (_lib.KeyFrame * max(len(frames), 1))()
    for i, (f, k) in enumerate(zip(frames, out)):
        desc[i] = _lib.KeyFrame(f.data_ptr(), k.data_ptr(), f.shape[0], f.shape[1])
    cnt, ptr = _count_ptr(stats)
    L = _lib.load()
    if frames:
        with torch.cuda.device(dev):
            _lib.check(L.tmfwm_sigma1_map_ragged_px(ctypes.addressof(desc), len(frames), block, px, _lib.MEM_DEVICE,
                                                    _stream(stream), code, ptr), "sigma1_map_ragged")
    if stats is not None:
        stats["lapack_blocks"] = int(cnt.value)
        stats["list_pass_blocks"] = int(L.tmfwm_last_list_pass_blocks()) if frames else 0
    return list(out)


def embed_with_key_ragged(frames, tiles, block: int = 8, alpha: float = 0.1, out=None, key_out=None, stream=None,
                          stats: dict | None = None, route: str = "hybrid"):
    """embed_ragged that also returns every frame's extraction key, by one set of launches
    (tmfwm_embed_key_ragged): (outs, keys), outs[i] the bytes of embed_ragged's output i, keys[i]
    the float32 (H_i // block, W_i // block) bits of sigma1_map_ragged's key i -- the key of the
    original frames[i], what extract_keyed_ragged takes with outs[i].  out and key_out are optional
    sequences of caller tensors (as embed_ragged's out and sigma1_map_ragged's out).  A frame
    smaller than a block gets its colour round trip and an empty key.  stats and route as
    embed_ragged's."""
    import ctypes

    frames = list(frames)
    alphas = _ragged_alphas(alpha, len(frames))
    frames, tiles, out, dev, code = _embed_ragged_args(frames, tiles, block, route, out)
    shapes = [(f.shape[0] // block, f.shape[1] // block) for f in frames]
    if key_out is None:  # float32 views of one uint8 allocation: its pieces start on 16-byte boundaries
        keys = [v.view(torch.float32).view(shapes[i]) for i, v in enumerate(
            _ragged_views([4 * a * b for a, b in shapes], lambda i: (4 * shapes[i][0] * shapes[i][1],), dev))] if frames else []
    else:
        keys = _check_ragged_out(key_out, shapes, torch.float32, dev, "key")
    desc = (_lib.EmbedKeyFrame * max(len(frames), 1))()
    for i, (f, t, o, k) in enumerate(zip(frames, tiles, out, keys)):
        desc[i] = _lib.EmbedKeyFrame(f.data_ptr(), o.data_ptr(), t.data_ptr(), k.data_ptr(), f.shape[0], f.shape[1])
    cnt, ptr = _count_ptr(stats)
    L = _lib.load()
    if frames:
        with torch.cuda.device(dev):
            if alphas is None:
                rc = L.tmfwm_embed_key_ragged(ctypes.addressof(desc), len(frames), block, float(alpha), _lib.MEM_DEVICE,
                                              _stream(stream), code, ptr)
            else:
                rc = L.tmfwm_embed_key_ragged_alphas(ctypes.addressof(desc), ctypes.addressof(alphas), len(frames), block,
                                                     _lib.MEM_DEVICE, _stream(stream), code, ptr)
            _lib.check(rc, "embed_with_key_ragged")
    if stats is not None:
        stats["lapack_blocks"] = int(cnt.value)
        stats["list_pass_blocks"] = int(L.tmfwm_last_list_pass_blocks()) if frames else 0
    return list(out), list(keys)


def embed_with_key_ragged_rank1(frames, tiles, block: int = 8, alpha: float = 0.1, out=None, key_out=None, stream=None,
                                stats: dict | None = None, route: str = "rank1"):
    """embed_with_key_ragged on every route (tmfwm_embed_key_ragged_rank1): on "rank1" and
    "rank1_reference" embed_ragged_rank1's passes and then sigma1_map_ragged's in the one call
    (the counts are the sums over both); "hybrid" and "reference" are embed_with_key_ragged itself.
    Arguments, checks and the return value are embed_with_key_ragged's."""
    import ctypes

    frames = list(frames)
    alphas = _ragged_alphas(alpha, len(frames))
    frames, tiles, out, dev, code = _embed_ragged_args(frames, tiles, block, route, out, rank1_routes=True)
    shapes = [(f.shape[0] // block, f.shape[1] // block) for f in frames]
    if key_out is None:  # float32 views of one uint8 allocation: its pieces start on 16-byte boundaries
        keys = [v.view(torch.float32).view(shapes[i]) for i, v in enumerate(
            _ragged_views([4 * a * b for a, b in shapes], lambda i: (4 * shapes[i][0] * shapes[i][1],), dev))] if frames else []
    else:
        keys = _check_ragged_out(key_out, shapes, torch.float32, dev, "key")
    desc = (_lib.EmbedKeyFrame * max(len(frames), 1))()
    for i, (f, t, o, k) in enumerate(zip(frames, tiles, out, keys)):
        desc[i] = _lib.EmbedKeyFrame(f.data_ptr(), o.data_ptr(), t.data_ptr(), k.data_ptr(), f.shape[0], f.shape[1])
    cnt, ptr = _count_ptr(stats)
    L = _lib.load()
    if frames:
        with torch.cuda.device(dev):
            if alphas is None:
                rc = L.tmfwm_embed_key_ragged_rank1(ctypes.addressof(desc), len(frames), block, float(alpha), _lib.MEM_DEVICE,
                                                    _stream(stream), code, ptr)
            else:
                rc = L.tmfwm_embed_key_ragged_alphas(ctypes.addressof(desc), ctypes.addressof(alphas), len(frames), block,
                                                     _lib.MEM_DEVICE, _stream(stream), code, ptr)
            _lib.check(rc, "embed_with_key_ragged_rank1")
    if stats is not None:
        stats["lapack_blocks"] = int(cnt.value)
        stats["list_pass_blocks"] = int(L.tmfwm_last_list_pass_blocks()) if frames else 0
    return list(out), list(keys)


def extract_keyed_ragged(wframes, keys, block: int = 8, alpha: float = 0.1, out=None, stream=None, stats: dict | None = None,
                         route: str = "hybrid") -> list:
    """extract_ragged without the original frames (tmfwm_extract_keyed_ragged): keys[i] is the
    float32 (H_i // block, W_i // block) sigma1 map of wframes[i]'s original; the same tensor may
    appear several times (one original, many watermarked copies).  Returns per-frame uint8 tiles,
    views of one device allocation (or `out`); tile i is the bytes of
    extract_keyed(wframes[i][None], keys[i], ...)[0], which are extract_batch's with the original.
    A key belongs to one block size and one image size.  The frames are (H_i, W_i, 3), or all of
    them (H_i, W_i, 4) R G B pad, read in place.  stats and route as sigma1_map_ragged's."""
    import ctypes

    if block not in SUPPORTED_BLOCK_SIZES:
        raise NotImplementedError(f"block {block}")
    code = _ragged_route(route)
    wframes, keys = list(wframes), list(keys)
    alphas = _ragged_alphas(alpha, len(wframes))
    if len(keys) != len(wframes):
        raise ValueError(f"{len(keys)} keys for {len(wframes)} frames")
    # what a key is, and whether it fits its frame, before any tensor's device is looked at
    for i, (w, k) in enumerate(zip(wframes, keys)):
        if not isinstance(k, torch.Tensor) or k.dtype != torch.float32:
            raise TypeError(f"keys[{i}] must be a float32 tensor")
        if isinstance(w, torch.Tensor) and w.dim() == 3 and tuple(k.shape) != (w.shape[0] // block, w.shape[1] // block):
            raise ValueError(f"keys[{i}] must be {(w.shape[0] // block, w.shape[1] // block)} for block {block} and a "
                             f"{w.shape[1]}x{w.shape[0]} frame, got {tuple(k.shape)}: a key belongs to one block size and one image size")
    wframes, dev = _check_ragged(wframes, "wframes", px=(3, 4))
    px = int(wframes[0].shape[-1]) if wframes else 3
    shapes = [(w.shape[0] // block, w.shape[1] // block) for w in wframes]
    for i, k in enumerate(keys):
        if k.device != dev or not k.is_contiguous():
            raise ValueError(f"keys[{i}] must be contiguous and on {dev}")
    if out is None:
        out = _ragged_views([a * b for a, b in shapes], lambda i: shapes[i], dev) if wframes else []
    else:
        out = _check_ragged_out(out, shapes, torch.uint8, dev, "tile")
    desc = (_lib.KeyedFrame * max(len(wframes), 1))()
    for i, (w, k, t) in enumerate(zip(wframes, keys, out)):
        desc[i] = _lib.KeyedFrame(w.data_ptr(), k.data_ptr(), t.data_ptr(), w.shape[0], w.shape[1])
    cnt, ptr = _count_ptr(stats)
    L = _lib.load()
    if wframes:
        with torch.cuda.device(dev):
            if alphas is None:
                rc = L.tmfwm_extract_keyed_ragged_px(ctypes.addressof(desc), len(wframes), block, float(alpha), px,
                                                     _lib.MEM_DEVICE, _stream(stream), code, ptr)
            else:
                rc = L.tmfwm_extract_keyed_ragged_alphas(ctypes.addressof(desc), ctypes.addressof(alphas), len(wframes), block, px,
                                                         _lib.MEM_DEVICE, _stream(stream), code, ptr)
            _lib.check(rc, "extract_keyed_ragged")
    if stats is not None:
        stats["lapack_blocks"] = int(cnt.value)
        stats["list_pass_blocks"] = int(L.tmfwm_last_list_pass_blocks()) if wframes else 0
    return list(out)


def synth_frames(n: int, height: int, width: int, seed: int = SEED_COVER, frame0: int = 0,
                 device: torch.device | str | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """Counter-based synthetic uint8 frames generated directly in HBM."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if out is None:
        out = torch.empty((n, height, width, 3), dtype=torch.uint8, device=dev)
    with torch.cuda.device(out.device):
        L = _lib.load()
        _lib.check(L.tmfwm_synth_frames(seed, frame0, n, height * width * 3, out.data_ptr(), _stream(None)), "synth_frames")
    return out


def synth_photo_frames(n: int, height: int, width: int, seed: int = SEED_COVER, frame0: int = 0,
                       device: torch.device | str | None = None, chunk: int = 16) -> torch.Tensor:
    """Camera-like synthetic uint8 frames (tests/lapack_path.photo_cover's recipe on the device:
    a low-pass field + gradients + fine grain, the decaying DCT spectra of natural images),
    generated `chunk` frames at a time with one generator seed per frame (seed + frame index)."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    out = torch.empty((n, height, width, 3), dtype=torch.uint8, device=dev)
    y = torch.linspace(0, 1, height, device=dev).view(1, height, 1, 1)
    x = torch.linspace(0, 1, width, device=dev).view(1, 1, width, 1)
    for c0 in range(0, n, chunk):
        k = min(chunk, n - c0)
        f = torch.empty((k, height // 16 + 2, width // 16 + 2, 3), device=dev)
        g = torch.Generator(device=dev)
        for i in range(k):
            g.manual_seed(seed + frame0 + c0 + i)
            f[i] = torch.randn(f.shape[1:], generator=g, device=dev)
        f = f.repeat_interleave(16, 1).repeat_interleave(16, 2)[:, :height, :width]
        for ax in (1, 2):
            for _ in range(2):
                f = (torch.roll(f, 5, ax) + torch.roll(f, -5, ax) + f) / 3.0
        img = 128 + 45 * f + 60 * (x - 0.5) + 30 * (y - 0.5)
        g.manual_seed(seed + frame0 + c0 + 0x9E3779B9)
        img += 2.0 * torch.randn(img.shape, generator=g, device=dev)
        out[c0:c0 + k] = img.clamp_(0, 255).to(torch.uint8)
    return out


def synth_qr_tile(nbh: int, nbw: int, seed: int = SEED_WATERMARK, device=None) -> torch.Tensor:
    """The app's watermark tile: a QR code of a 48-byte payload (an AES-CBC ciphertext's size:
    IV + two blocks, base64 in the symbol, level H) rendered by text_to_qrcode (300 x 300) and
    resized to the block grid by resize_watermark with preserve_ratio=True, as the embed page does
    (embed_watermark_page.py:492-531; modules/qrcode_generator.py:10-44): 0 / 255 modules with
    LANCZOS edges, centred on a white canvas."""
    import numpy as np  # noqa: PLC0415

    from . import qrcode_generator, watermarking  # noqa: PLC0415

    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    payload = np.random.default_rng(seed).integers(0, 256, 48).astype(np.uint8).tobytes()
    img = qrcode_generator.text_to_qrcode(payload)
    with torch.cuda.device(dev):
        t = np.asarray(watermarking.resize_watermark(img, nbh, nbw, preserve_ratio=True), dtype=np.uint8)
    return torch.from_numpy(np.ascontiguousarray(t)).to(dev)


def synth_tile(nbh: int, nbw: int, seed: int = SEED_WATERMARK, device=None) -> torch.Tensor:
    """Synthetic watermark tile: the same generator over an nbh x nbw byte plane."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    out = torch.empty((nbh, nbw), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        L = _lib.load()
        _lib.check(L.tmfwm_synth_frames(seed, 0, 1, nbh * nbw, out.data_ptr(), _stream(None)), "synth_tile")
    return out


def svd_blocks(D: torch.Tensor):
    """SVD stage alone on (n, b, b) float32 blocks: (U, S, Vt, sweeps) as the reference consumes them."""
    if not D.is_cuda or D.dtype != torch.float32 or D.dim() != 3 or D.shape[1] != D.shape[2]:
        raise ValueError("D must be (n, b, b) float32 on the GPU")
    D = D.contiguous()
    n, b, _ = D.shape
    U = torch.empty_like(D)
    Vt = torch.empty_like(D)
    S = torch.empty((n, b), dtype=torch.float32, device=D.device)
    sw = torch.empty((n,), dtype=torch.int32, device=D.device)
    with torch.cuda.device(D.device):
        L = _lib.load()
        _lib.check(L.tmfwm_svd_blocks(D.data_ptr(), n, b, U.data_ptr(), S.data_ptr(), Vt.data_ptr(), sw.data_ptr(),
                                      _lib.MEM_DEVICE, _stream(None)), "svd_blocks")
    return U, S, Vt, sw


def lapack_svd_blocks(D: torch.Tensor, want_vectors: bool = True):
    """np.linalg.svd on the dgesdd route (the reference's arithmetic) for (n, b, b) float32
    blocks on the GPU: (U, S, Vt), or (None, S, None) without vectors."""
    if not D.is_cuda or D.dtype != torch.float32 or D.dim() != 3 or D.shape[1] != D.shape[2]:
        raise ValueError("D must be (n, b, b) float32 on the GPU")
    D = D.contiguous()
    n, b, _ = D.shape
    S = torch.empty((n, b), dtype=torch.float32, device=D.device)
    U = torch.empty_like(D) if want_vectors else None
    Vt = torch.empty_like(D) if want_vectors else None
    with torch.cuda.device(D.device):
        L = _lib.load()
        _lib.check(L.tmfwm_lapack_svd_blocks(D.data_ptr(), n, b, U.data_ptr() if want_vectors else None, S.data_ptr(),
                                             Vt.data_ptr() if want_vectors else None, int(want_vectors), _lib.MEM_DEVICE,
                                             _stream(None)), "lapack_svd_blocks")
    return U, S, Vt


def prepare_tile(watermark_l: torch.Tensor, tile_height: int, tile_width: int, preserve_ratio: bool = False,
                 out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
    """resize_watermark (watermarking.py:105-130) on a device-resident (h, w) uint8 grey
    watermark: Pillow-exact LANCZOS resample (+ centred paste on white when
    preserve_ratio).  Synchronises the stream (the resample tables come from the host)."""
    if not watermark_l.is_cuda or watermark_l.dtype != torch.uint8 or watermark_l.dim() != 2:
        raise ValueError("watermark_l must be a (h, w) uint8 GPU tensor")
    watermark_l = watermark_l.contiguous()
    if out is None:
        out = torch.empty((tile_height, tile_width), dtype=torch.uint8, device=watermark_l.device)
    elif tuple(out.shape) != (tile_height, tile_width) or out.dtype != torch.uint8 or not out.is_contiguous():
        raise ValueError("out must be a contiguous (tile_height, tile_width) uint8 tensor")
    with torch.cuda.device(watermark_l.device):
        L = _lib.load()
        _lib.check(L.tmfwm_prepare_tile(watermark_l.data_ptr(), watermark_l.shape[0], watermark_l.shape[1], tile_height,
                                        tile_width, int(bool(preserve_ratio)), out.data_ptr(), _lib.MEM_DEVICE, _stream(stream)),
                   "prepare_tile")
    return out


def prepare_tiles(watermarks_l: torch.Tensor, tile_height: int, tile_width: int, preserve_ratio: bool = False,
                  out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
    """prepare_tile for a batch: (N, h, w) uint8 grey watermarks of one size on the GPU ->
    (N, tile_height, tile_width) tiles, tile i the bytes of prepare_tile(watermarks_l[i], ...).
    One table upload and one launch per resample pass for the whole batch; synchronises the
    stream once (the resample tables come from the host)."""
    if not watermarks_l.is_cuda or watermarks_l.dtype != torch.uint8 or watermarks_l.dim() != 3:
        raise ValueError("watermarks_l must be a (N, h, w) uint8 GPU tensor")
    watermarks_l = watermarks_l.contiguous()
    n, h, w = watermarks_l.shape
    if out is None:
        out = torch.empty((n, tile_height, tile_width), dtype=torch.uint8, device=watermarks_l.device)
    elif (tuple(out.shape) != (n, tile_height, tile_width) or out.dtype != torch.uint8 or not out.is_contiguous()
          or out.device != watermarks_l.device):
        raise ValueError("out must be a contiguous (N, tile_height, tile_width) uint8 tensor on the watermarks' device")
    with torch.cuda.device(watermarks_l.device):
        L = _lib.load()
        _lib.check(L.tmfwm_prepare_tiles(watermarks_l.data_ptr(), n, h, w, h * w, tile_height, tile_width,
                                         int(bool(preserve_ratio)), out.data_ptr(), tile_height * tile_width, _lib.MEM_DEVICE,
                                         _stream(stream)), "prepare_tiles")
    return out


def prepare_tiles_ragged(watermarks, sizes, preserve_ratio: bool = False, out=None, stream=None) -> list:
    """prepare_tile for jobs of mixed sizes by one set of launches (tmfwm_prepare_tiles_ragged):
    watermarks is a list of contiguous (h, w) uint8 GPU tensors, one per entry of sizes, or a single tensor
    used for every size; sizes is a list of (tile_height, tile_width).  Returns one
    (tile_height, tile_width) tile per job, views of one device allocation (or `out`, a list of
    contiguous tensors of those shapes on the watermarks' device); tile i is the bytes of
    prepare_tile(watermarks[i], *sizes[i], preserve_ratio).  Each distinct resample axis of the
    call is built once and everything goes up in one copy; the call does not synchronise."""
    import ctypes

    sizes = [(int(th), int(tw)) for th, tw in sizes]
    if isinstance(watermarks, torch.Tensor):
        watermarks = [watermarks] * len(sizes)
    watermarks = list(watermarks)
    if len(watermarks) != len(sizes):
        raise ValueError(f"{len(watermarks)} watermarks for {len(sizes)} sizes")
    dev = None
    for i, w in enumerate(watermarks):
        if not isinstance(w, torch.Tensor) or not w.is_cuda or w.dtype != torch.uint8 or w.dim() != 2 or not w.is_contiguous():
            raise ValueError(f"watermarks[{i}] must be a contiguous (h, w) uint8 GPU tensor")
        dev = w.device if dev is None else dev
        if w.device != dev:
            raise ValueError(f"watermarks[{i}] is on {w.device}, the call's other tensors on {dev}")
    for i, (th, tw) in enumerate(sizes):
        if th <= 0 or tw <= 0:
            raise ValueError(f"sizes[{i}] = {(th, tw)}: height and width must be > 0")
    if not sizes:
        return []
    if out is None:
        out = _ragged_views([th * tw for th, tw in sizes], lambda i: sizes[i], dev)
    else:
        out = list(out)
        if len(out) != len(sizes):
            raise ValueError("out must hold one tile per job")
        for i, t in enumerate(out):
            if (not isinstance(t, torch.Tensor) or tuple(t.shape) != sizes[i] or t.dtype != torch.uint8 or t.device != dev
                    or not t.is_contiguous()):
                raise ValueError(f"out[{i}] must be a contiguous {sizes[i]} uint8 tensor on {dev}")
    desc = (_lib.TileJob * len(sizes))()
    for i, (w, t) in enumerate(zip(watermarks, out)):
        desc[i] = _lib.TileJob(w.data_ptr(), t.data_ptr(), w.shape[0], w.shape[1], sizes[i][0], sizes[i][1])
    with torch.cuda.device(dev):
        L = _lib.load()
        _lib.check(L.tmfwm_prepare_tiles_ragged(ctypes.addressof(desc), len(sizes), int(bool(preserve_ratio)), _lib.MEM_DEVICE,
                                                _stream(stream)), "prepare_tiles_ragged")
    return list(out)
