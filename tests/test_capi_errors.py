"""The error contract of the batch entry points of the C ABI, replayed from a recorded table.

tests/golden/capi_errors.json (tests/golden/gen_capi_errors.py) holds under `bases` a valid
call of each entry point as plain data and, per row, the base it starts from, the arguments it
changes and the (code, tmfwm_last_error() text, value left in *n_lapack_blocks) the library
answered when the table was recorded (`"match": "prefix"`: the text's stable beginning).
Every row is an invalid call that validation refuses: no row launches a kernel.  Section
`before_device` fails before the library looks for a device, so it gives the same answer with
and without a GPU; section `after_device` fails behind that check and needs one.
"""
import ctypes
import json
import math
import os

import pytest

from thatsmyface_amd import _lib

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "capi_errors.json")
BUF_BYTES = 8192  # every named buffer: room for 2 RGBX frames of 16x16 and then some
COUNT_SENTINEL = 77  # *n_lapack_blocks before the call

# parameter names of include/tmfwm.h, in call order; "ptr" parameters take buffer tokens
ORDER = {
    "tmfwm_embed_route": ["rgb:ptr", "n_frames", "height", "width", "frame_stride", "wm_tile:ptr", "block", "alpha:f", "out:ptr",
                          "mem_kind", "stream:ptr", "route", "count:ptr"],
    "tmfwm_extract_route": ["wm_rgb:ptr", "orig_rgb:ptr", "n_frames", "height", "width", "frame_stride", "block", "alpha:f",
                            "out_tiles:ptr", "mem_kind", "stream:ptr", "route", "count:ptr"],
    "tmfwm_embed_tiles": ["rgb:ptr", "in_pixel_bytes", "in_frame_stride", "n_frames", "height", "width", "wm_tiles:ptr",
                          "tile_stride", "block", "alpha:f", "out:ptr", "out_pixel_bytes", "out_frame_stride", "mem_kind",
                          "stream:ptr", "route", "count:ptr"],
    "tmfwm_embed_px": ["rgb:ptr", "in_pixel_bytes", "in_frame_stride", "n_frames", "height", "width", "wm_tile:ptr", "block",
                       "alpha:f", "out:ptr", "out_pixel_bytes", "out_frame_stride", "mem_kind", "stream:ptr", "route", "count:ptr"],
    "tmfwm_extract_px": ["wm_rgb:ptr", "wm_pixel_bytes", "wm_frame_stride", "orig_rgb:ptr", "orig_pixel_bytes",
                         "orig_frame_stride", "n_frames", "height", "width", "block", "alpha:f", "out_tiles:ptr", "mem_kind",
                         "stream:ptr", "route", "count:ptr"],
    "tmfwm_sigma1_map": ["rgb:ptr", "n_frames", "height", "width", "frame_stride", "block", "out_key:ptr", "mem_kind",
                         "stream:ptr", "route", "count:ptr"],
    "tmfwm_extract_keyed": ["wm_rgb:ptr", "n_frames", "height", "width", "frame_stride", "key:ptr", "key_stride", "block",
                            "alpha:f", "out_tiles:ptr", "mem_kind", "stream:ptr", "route", "count:ptr"],
    # frames: "null" or a list of [pointer, pointer, pointer, height, width] in the descriptor's field order
    "tmfwm_embed_ragged": ["frames:desc", "n_frames", "block", "alpha:f", "mem_kind", "stream:ptr", "route", "count:ptr"],
    "tmfwm_extract_ragged": ["frames:desc", "n_frames", "block", "alpha:f", "mem_kind", "stream:ptr", "route", "count:ptr"],
}


class Buffers:
    """Named zeroed buffers of BUF_BYTES: token "h:<name>[+off]" is host memory, "d:<name>[+off]"
    device memory (allocated on first use), "null" a NULL pointer."""

    def __init__(self):
        self.host, self.dev = {}, {}

    def address(self, token):
        if token == "null":
            return None
        kind, _, rest = token.partition(":")
        name, _, off = rest.partition("+")
        if kind == "h":
            buf = self.host.setdefault(name, (ctypes.c_uint8 * BUF_BYTES)())
            base = ctypes.addressof(buf)
        else:
            assert kind == "d", token
            if name not in self.dev:
                import torch

                self.dev[name] = torch.zeros(BUF_BYTES, dtype=torch.uint8, device="cuda")
            base = self.dev[name].data_ptr()
        return base + int(off or 0)


def to_float(v):
    return float(v) if isinstance(v, str) else v  # "nan" / "inf": JSON has no such numbers


def replay(row, bufs):
    """Make the call a row describes -> (code, message, *n_lapack_blocks afterwards or None)."""
    L = _lib.load()
    args, keep = [], []
    count = None
    for spec in ORDER[row["fn"]]:
        name, _, kind = spec.partition(":")
        v = row["args"][name]
        if name == "count":
            if v:
                count = ctypes.c_int64(COUNT_SENTINEL)
                args.append(ctypes.addressof(count))
            else:
                args.append(None)
        elif kind == "ptr":
            args.append(bufs.address(v))
        elif kind == "f":
            args.append(to_float(v))
        elif kind == "desc":
            if v == "null":
                args.append(None)
                continue
            cls = _lib.EmbedFrame if row["fn"] == "tmfwm_embed_ragged" else _lib.ExtractFrame
            arr = (cls * max(1, len(v)))()
            for i, (p0, p1, p2, h, w) in enumerate(v):
                arr[i] = cls(bufs.address(p0), bufs.address(p1), bufs.address(p2), h, w)
            keep.append(arr)
            args.append(ctypes.addressof(arr))
        else:
            args.append(v)
    code = getattr(L, row["fn"])(*args)
    return code, _lib.last_error(), None if count is None else count.value


def call_of(bases, row):
    base = bases[row["base"]]
    return {"fn": base["fn"], "args": {**base["args"], **row["change"]}}


def load_table():
    with open(TABLE) as f:
        return json.load(f)


def write_table(table, path):  # one row per line
    with open(path, "w") as f:
        f.write("{\n")
        for section in ("bases", "before_device", "after_device"):
            items = table[section]
            lines = [f"{json.dumps(k)}: {json.dumps(v)}" for k, v in items.items()] if section == "bases" else [json.dumps(r) for r in items]
            body = ",\n".join("  " + ln for ln in lines)
            opener, closer = ("{", "}") if section == "bases" else ("[", "]")
            f.write(f' "{section}": {opener}\n{body}\n {closer}' + ("\n" if section == "after_device" else ",\n"))
        f.write("}\n")


def check_section(section):
    table = load_table()
    rows = table[section]
    assert len(rows) >= 20, "the recorded table is missing"
    bufs = Buffers()
    bad = []
    for i, row in enumerate(rows):
        code, msg, count_after = replay(call_of(table["bases"], row), bufs)
        ok = code == row["code"] and count_after == row["count_after"]
        ok = ok and (msg.startswith(row["message"]) if row.get("match") == "prefix" else msg == row["message"])
        if not ok:
            bad.append(f"row {i} {row['base']} [{row['case']}]: got ({code}, {msg!r}, count {count_after}), "
                       f"recorded ({row['code']}, {row['message']!r}, count {row['count_after']})")
    assert not bad, "\n".join(bad)


def test_rows_are_well_formed():
    t = load_table()
    for section in ("before_device", "after_device"):
        for row in t[section]:
            call = call_of(t["bases"], row)
            assert row["code"] != 0 and row["message"] and row["change"], row
            assert row.get("match", "prefix") == "prefix", row
            assert set(call["args"]) == {s.partition(":")[0] for s in ORDER[call["fn"]]}, row
            a = call["args"].get("alpha")
            assert a is None or isinstance(a, str) or math.isfinite(a), row
        assert {t["bases"][r["base"]]["fn"] for r in t[section]} == set(ORDER)


def test_errors_before_the_device_check():
    check_section("before_device")


@pytest.mark.gpu
def test_errors_after_the_device_check():
    check_section("after_device")
