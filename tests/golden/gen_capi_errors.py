#!/usr/bin/env python3
"""Records tests/golden/capi_errors.json, the error contract of the batch entry points that
tests/test_capi_errors.py replays: run it on the commit whose answers are to be pinned.

    python tests/golden/gen_capi_errors.py before [OUT.json]   # a machine without a GPU
    python tests/golden/gen_capi_errors.py after [OUT.json]    # a machine with a GPU

The table's `bases` are valid host-memory calls; a row names its base and the arguments it
changes.  `before` makes every call of cases() and keeps those refused before the library looks for a
device (on a machine without a GPU the others answer TMFWM_ERR_NODEVICE).  `after` makes the
calls that `before` did not keep and records what the validation behind the device check
answers; every one of them must be refused (a call that succeeded would have launched kernels:
the generator stops).  Rows whose message quotes a driver string or a memory type are kept as
the stable prefix, `"match": "prefix"`.

*n_lapack_blocks holds 77 before each call: `count_after` 77 means the call returned before it
zeroed the count (a route outside the enumeration does), 0 that it failed behind that point.

16x16 frames, b = 8, 2x2 tiles, 2 frames; every pointer token names a zeroed 8 KiB buffer.
"""
import copy
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import test_capi_errors as T  # noqa: E402

from thatsmyface_amd import _lib  # noqa: E402

F3, F4, KEY = 16 * 16 * 3, 16 * 16 * 4, 2 * 2 * 4
COMMON = {"n_frames": 2, "block": 8, "alpha": 0.1, "mem_kind": 0, "stream": "null", "route": 0, "count": True}
SIZE = {"height": 16, "width": 16}

# variant -> (entry point, valid host-memory arguments)
BASES = {
    "embed_route": ("tmfwm_embed_route", {"rgb": "h:a", "frame_stride": F3, "wm_tile": "h:t", "out": "h:o", **SIZE}),
    "extract_route": ("tmfwm_extract_route", {"wm_rgb": "h:a", "orig_rgb": "h:b", "frame_stride": F3, "out_tiles": "h:o", **SIZE}),
    "embed_tiles/44": ("tmfwm_embed_tiles", {"rgb": "h:a", "in_pixel_bytes": 4, "in_frame_stride": F4, "wm_tiles": "h:t",
                                             "tile_stride": 4, "out": "h:o", "out_pixel_bytes": 4, "out_frame_stride": F4, **SIZE}),
    "embed_tiles/33": ("tmfwm_embed_tiles", {"rgb": "h:a", "in_pixel_bytes": 3, "in_frame_stride": F3, "wm_tiles": "h:t",
                                             "tile_stride": 4, "out": "h:o", "out_pixel_bytes": 3, "out_frame_stride": F3, **SIZE}),
    "embed_px/44": ("tmfwm_embed_px", {"rgb": "h:a", "in_pixel_bytes": 4, "in_frame_stride": F4, "wm_tile": "h:t", "out": "h:o",
                                       "out_pixel_bytes": 4, "out_frame_stride": F4, **SIZE}),
    "embed_px/33": ("tmfwm_embed_px", {"rgb": "h:a", "in_pixel_bytes": 3, "in_frame_stride": F3, "wm_tile": "h:t", "out": "h:o",
                                       "out_pixel_bytes": 3, "out_frame_stride": F3, **SIZE}),
    "extract_px/43": ("tmfwm_extract_px", {"wm_rgb": "h:a", "wm_pixel_bytes": 4, "wm_frame_stride": F4, "orig_rgb": "h:b",
                                           "orig_pixel_bytes": 3, "orig_frame_stride": F3, "out_tiles": "h:o", **SIZE}),
    "extract_px/33": ("tmfwm_extract_px", {"wm_rgb": "h:a", "wm_pixel_bytes": 3, "wm_frame_stride": F3, "orig_rgb": "h:b",
                                           "orig_pixel_bytes": 3, "orig_frame_stride": F3, "out_tiles": "h:o", **SIZE}),
    "sigma1_map": ("tmfwm_sigma1_map", {"rgb": "h:a", "frame_stride": F3, "out_key": "h:k", **SIZE}),
    "extract_keyed": ("tmfwm_extract_keyed", {"wm_rgb": "h:a", "frame_stride": F3, "key": "h:k", "key_stride": KEY,
                                              "out_tiles": "h:o", **SIZE}),
    # descriptors in field order: embed rgb, out, wm_tile; extract wm_rgb, orig_rgb, out_tile
    "embed_ragged": ("tmfwm_embed_ragged", {"frames": [["h:a", "h:o", "h:t", 16, 16], ["h:b", "h:p", "h:u", 16, 16]]}),
    "extract_ragged": ("tmfwm_extract_ragged", {"frames": [["h:a", "h:b", "h:o", 16, 16], ["h:c", "h:d", "h:p", 16, 16]]}),
}
EXTRACTS = {"extract_route", "extract_px/43", "extract_px/33", "extract_keyed", "extract_ragged"}
NO_ALPHA = {"sigma1_map"}
OUTPUTS = {"out", "out_tiles", "out_key"}
# tmfwm_embed_px with RGBX frames has no tile-overlap rule; the 3 -> 3 calls are tmfwm_embed_route's
TILE_RULE = {"embed_route", "embed_tiles/44", "embed_tiles/33", "embed_px/33"}
# the 3 -> 3 forms hand over to tmfwm_embed_route / tmfwm_extract_route: only what shows the hand-over
DELEGATED = {"embed_tiles/33", "embed_px/33", "extract_px/33"}
DELEGATED_CASES = {"route 4", "block 7", "3 -> 3 with two strides", "3 -> 3 with two strides and route 4", "tile_stride -1",
                   "in_pixel_bytes 5", "alpha nan", "mem_kind 7", "host: out NULL", "host: out_tiles NULL", "device: out is rgb",
                   "device: out is wm_tile", "device: out is wm_tiles", "device: out_tiles is orig_rgb"}


def base_args(variant):
    fn, own = BASES[variant]
    args = {**COMMON, **copy.deepcopy(own)}
    if variant in NO_ALPHA:
        del args["alpha"]
    return fn, args


def pointer_params(fn):
    return [s.partition(":")[0] for s in T.ORDER[fn] if s.endswith(":ptr") and s.partition(":")[0] not in ("stream", "count")]


def on_device(args, fn):
    a = copy.deepcopy(args)
    a["mem_kind"] = 1
    for p in pointer_params(fn):
        a[p] = "d:" + a[p][2:]
    if "frames" in a:
        a["frames"] = [["d:" + t[2:] for t in f[:3]] + f[3:] for f in a["frames"]]
    return a


def mutations(variant):
    """(case name, arguments changed from the valid call, prefix match) of one variant."""
    fn, args = base_args(variant)
    ragged = "frames" in args
    m = []
    add = lambda name, change, prefix=False: m.append((name, change, prefix))  # noqa: E731
    frames = lambda i, j, v: {"frames": [[v if (a, b) == (i, j) else x for b, x in enumerate(f)]  # noqa: E731
                                         for a, f in enumerate(args.get("frames", []))]}
    for r in (-1, 4):
        add(f"route {r}", {"route": r})
    add("block 7, no count pointer", {"block": 7, "count": False})
    if ragged:
        for r in (2, 3):
            add(f"route {r} (rank-1)", {"route": r})
    add("n_frames -1", {"n_frames": -1})
    for b in (2, 7, 18):
        add(f"block {b}", {"block": b})
    if ragged:
        add("frame 1 height -1", frames(1, 3, -1))
        add("frame 1 width -1", frames(1, 4, -1))
        add("frames NULL", {"frames": "null"})
        for j in range(3):
            add(f"frame 1 pointer {j} NULL", frames(1, j, "null"))
        add("frame 1 with more than 2^31 - 1 blocks", {"block": 4, "frames": [args["frames"][0], args["frames"][1][:3] + [185368, 185368]]})
        add("route 4 and block 7", {"route": 4, "block": 7})
        add("block 7 and frame 1 height -1", {"block": 7, **frames(1, 3, -1)})
        add("block 7 and alpha nan", {"block": 7, "alpha": "nan"})
    else:
        add("height -1", {"height": -1})
        add("width -1", {"width": -1})
    strides = [p for p in args if p.endswith("frame_stride")]
    for p in strides:
        add(f"{p} one byte short", {p: args[p] - 1})
    for p in [p for p in args if p.endswith("pixel_bytes")]:
        for v in (2, 5):
            add(f"{p} {v}", {p: v})
    if variant in ("embed_tiles/33", "embed_px/33"):
        add("3 -> 3 with two strides", {"out_frame_stride": F3 + 4})
        add("3 -> 3 with two strides and route 4", {"out_frame_stride": F3 + 4, "route": 4})
    if "tile_stride" in args:
        for v in (-1, 3):
            add(f"tile_stride {v}", {"tile_stride": v})
    if "key_stride" in args:
        for v in (-4, 18, 12):
            add(f"key_stride {v}", {"key_stride": v})
    if "alpha" in args:
        for v in (("nan", 0.0) if variant in EXTRACTS else ("nan", "inf")):
            add(f"alpha {v}", {"alpha": v})
    # which of two wrong arguments is reported
    if not ragged:
        add("route 4 and block 7", {"route": 4, "block": 7})
        add("block 7 and stride short", {"block": 7, strides[0]: args[strides[0]] - 1})
        if "alpha" in args:
            add("stride short and alpha nan", {strides[-1]: args[strides[-1]] - 1, "alpha": "nan"})
    if "tile_stride" in args and "in_pixel_bytes" in args:
        add("pixel bytes 5 and tile_stride -1", {"out_pixel_bytes": 5, "tile_stride": -1})
        add("tile_stride -1 and alpha nan", {"tile_stride": -1, "alpha": "nan"})
    if "key_stride" in args:
        add("key_stride 18 and alpha 0", {"key_stride": 18, "alpha": 0.0})
        add("key_stride 18 and alpha nan", {"key_stride": 18, "alpha": "nan"})

    # ---- refused behind the device check (all of them before any launch)
    add("mem_kind 7", {"mem_kind": 7})
    dev = on_device(args, fn)
    if ragged:
        add("host frames as device memory", {"mem_kind": 1}, True)
        out_j = 1 if fn == "tmfwm_embed_ragged" else 2
        over_input = copy.deepcopy(dev["frames"])
        over_input[1][out_j] = over_input[0][0]
        add("device: frame 1 writes over frame 0's input", {**dev, "frames": over_input})
        same_out = copy.deepcopy(dev["frames"])
        same_out[1][out_j] = same_out[0][out_j]
        add("device: both frames write one buffer", {**dev, "frames": same_out})
        return fn, args, m
    ptrs = pointer_params(fn)
    add("host arrays as device memory", {"mem_kind": 1}, True)
    for p in ptrs:
        # tmfwm_extract_px packs RGBX watermarked frames before it looks at orig_rgb: not a row
        if variant == "extract_px/43" and p == "orig_rgb":
            continue
        add(f"host: {p} NULL", {p: "null"})
        add(f"device: {p} NULL", {**dev, p: "null"})
        add(f"device: {p} a host array", {**dev, p: args[p]}, True)
    out = [p for p in ptrs if p in OUTPUTS][0]
    ins = [p for p in ptrs if p not in OUTPUTS]
    for p in ins:
        if p in ("wm_tile", "wm_tiles") and variant not in TILE_RULE:
            continue
        add(f"device: {out} is {p}", {**dev, out: dev[p]})
    if "key" in args:
        add("device: key not 4-byte aligned", {**dev, "key": dev["key"] + "+2"})
    if "out_key" in args:
        add("device: out_key not 4-byte aligned", {**dev, "out_key": dev["out_key"] + "+2"})
    return fn, args, m


def cases():
    """Rows without their answers: the base variant, the case's name, the arguments it changes."""
    for variant in BASES:
        fn, args, muts = mutations(variant)
        for name, change, prefix in muts:
            if variant in DELEGATED and name not in DELEGATED_CASES:
                continue
            yield {"base": variant, "case": name, "change": {k: v for k, v in change.items() if args[k] != v}, "prefix": prefix}


def stable_prefix(msg):
    cut = msg.find(" is not ")
    assert cut >= 0, msg
    return msg[:cut + len(" is not ")]


def main():
    mode = sys.argv[1]
    path = sys.argv[2] if len(sys.argv) > 2 else T.TABLE
    table = {"before_device": [], "after_device": []}
    if os.path.exists(T.TABLE):
        table = T.load_table()
    table["bases"] = {v: dict(zip(("fn", "args"), base_args(v))) for v in BASES}
    kept = {(r["base"], r["case"]) for r in table["before_device"]}
    bufs = T.Buffers()
    rows = []
    for c in cases():
        if mode == "after" and (c["base"], c["case"]) in kept:
            continue
        if mode == "before" and '"d:' in json.dumps(c["change"]):
            continue  # device buffers: behind the device check by construction
        prefix = c.pop("prefix")
        code, msg, count_after = T.replay(T.call_of(table["bases"], c), bufs)
        if mode == "before" and code == _lib.ERR_NODEVICE:
            continue
        if code == 0 or code == _lib.ERR_NODEVICE:
            raise SystemExit(f"{c['base']}: {c['case']}: not refused by validation (code {code}, {msg!r})")
        rows.append({**c, "code": code, "message": stable_prefix(msg) if prefix else msg, "count_after": count_after,
                     **({"match": "prefix"} if prefix else {})})
    table["before_device" if mode == "before" else "after_device"] = rows
    T.write_table(table, path)
    print(f"{mode}: {len(rows)} rows -> {path}")


if __name__ == "__main__":
    main()
