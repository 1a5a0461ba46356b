"""Ragged tile preparation on the CPU: the C ABI of tmfwm_prepare_tiles_ragged (symbol, layout,
argument checks before the device), the Python layer's own checks, the pipeline's grouping, and the
plan plus the index arithmetic of both passes compiled for the host (tests/native/tile_plan_host.cpp
walks the two grids with the functions the kernels call) against the oracle's prepare_tile.  The
GPU run is tests/test_tiles_ragged_gpu.py."""
import ctypes
import io
import os
import shutil
import subprocess

import numpy as np
import pytest
from PIL import Image

from thatsmyface_amd import _lib, pipeline
from tiles_ragged_jobs import ERROR_JOBS, JOBS, distinct_axes, expected, resized, watermarks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "tile_plan_host.cpp")
HDR = os.path.join(ROOT, "thatsmyface_amd", "csrc", "tmfwm_tile_plan.h")
OUT = os.path.join(ROOT, "tests", "_build", "libtile_plan_host.so")
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall"]


def _desc(rows):
    d = (_lib.TileJob * max(len(rows), 1))()
    for i, r in enumerate(rows):
        d[i] = _lib.TileJob(*r)
    return d


def _host_rows(jobs, wms=None):
    """(descriptor rows, watermark arrays, tile arrays) of host-memory jobs."""
    wms = wms or [np.full(wm, 200, np.uint8) for wm, _ in jobs]
    tiles = [np.full(t, 0x5A, np.uint8) for _, t in jobs]
    rows = [(w.ctypes.data, t.ctypes.data, w.shape[0], w.shape[1], t.shape[0], t.shape[1]) for w, t in zip(wms, tiles)]
    return rows, wms, tiles


def _call(rows, n=None, preserve=0, mem=_lib.MEM_HOST):
    d = _desc(rows)
    return _lib.load().tmfwm_prepare_tiles_ragged(ctypes.addressof(d), len(rows) if n is None else n, preserve, mem, None)


def test_symbol_signature_and_layout():
    L = _lib.load()
    assert hasattr(L, "tmfwm_prepare_tiles_ragged")
    res, args = _lib.SIGNATURES["tmfwm_prepare_tiles_ragged"]
    assert res is ctypes.c_int and len(args) == 5
    assert ctypes.sizeof(_lib.TileJob) == 32
    assert [f[0] for f in _lib.TileJob._fields_] == ["wm", "tile", "wm_height", "wm_width", "tile_height", "tile_width"]
    assert [getattr(_lib.TileJob, n).offset for n in ("wm", "tile", "wm_height", "wm_width", "tile_height", "tile_width")] == [
        0, 8, 16, 20, 24, 28]
    assert L.tmfwm_abi_version() == _lib.ABI_VERSION == 10


def test_argument_checks_before_the_device():
    L = _lib.load()
    rows, _wms, tiles = _host_rows([((29, 31), (17, 25)), ((29, 31), (40, 31)), ((17, 25), (9, 9))])
    assert _call(rows, n=-1) == _lib.ERR_INVALID
    assert L.tmfwm_prepare_tiles_ragged(None, 2, 0, _lib.MEM_HOST, None) == _lib.ERR_INVALID
    assert "NULL" in _lib.last_error()
    assert _call(rows, mem=7) == _lib.ERR_INVALID
    assert "mem_kind" in _lib.last_error()
    for mem in (_lib.MEM_HOST, _lib.MEM_DEVICE):  # inside the second job, before any pointer is looked at
        for field in range(2, 6):
            for v in (0, -3):
                bad = [list(r) for r in rows]
                bad[1][field] = v
                assert _call(bad, mem=mem) == _lib.ERR_INVALID, (mem, field, v)
                assert "job 1" in _lib.last_error(), _lib.last_error()
        for field in (0, 1):
            bad = [list(r) for r in rows]
            bad[1][field] = None
            assert _call(bad, mem=mem) == _lib.ERR_INVALID, (mem, field)
            assert "NULL" in _lib.last_error() and "job 1" in _lib.last_error(), _lib.last_error()
    # the error jobs: valid without preserve_ratio, an empty resized size with it
    for k, job in enumerate(ERROR_JOBS):
        jobs = [JOBS[4], JOBS[6], job] if k == 0 else [JOBS[4], job, JOBS[6]]
        erows, _w, etiles = _host_rows(jobs)
        for mem in (_lib.MEM_HOST, _lib.MEM_DEVICE):
            assert _call(erows, preserve=1, mem=mem) == _lib.ERR_INVALID
            assert f"job {2 - k}" in _lib.last_error(), _lib.last_error()
        assert all((t == 0x5A).all() for t in etiles)  # nothing written
        with pytest.raises(ValueError):  # the oracle refuses it too
            from oracle import oracle as O

            O.prepare_tile(np.zeros(job[0], np.uint8), *job[1], True)
        rc = _call(erows, preserve=0)
        assert rc == (0 if _lib.device_count() > 0 else _lib.ERR_NODEVICE), _lib.last_error()
    assert all((t == 0x5A).all() for t in tiles)
    # valid calls: there is no CPU path
    want = 0 if _lib.device_count() > 0 else _lib.ERR_NODEVICE
    for preserve in (0, 1):
        assert _call(rows, preserve=preserve) == want, _lib.last_error()
    assert _call(rows, n=0) == want  # as tmfwm_prepare_tiles with n_wm == 0
    assert L.tmfwm_prepare_tiles_ragged(None, 0, 0, _lib.MEM_HOST, None) == want
    if want:
        assert "no HIP device" in _lib.last_error()


def test_python_layer_checks_come_before_the_library(monkeypatch):
    torch = pytest.importorskip("torch")
    from thatsmyface_amd import batch

    def no_library():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "load", no_library)
    cpu = [torch.zeros((29, 31), dtype=torch.uint8) for _ in range(3)]
    with pytest.raises(ValueError, match="GPU tensor"):
        batch.prepare_tiles_ragged(cpu, [(4, 4), (5, 5), (6, 6)])
    with pytest.raises(ValueError, match="GPU tensor"):
        batch.prepare_tiles_ragged(cpu[0], [(4, 4), (5, 5)])
    with pytest.raises(ValueError, match="3 watermarks for 2 sizes"):
        batch.prepare_tiles_ragged(cpu, [(4, 4), (5, 5)])
    with pytest.raises(ValueError, match="2 watermarks for 3 sizes"):
        batch.prepare_tiles_ragged(cpu[:2], [(4, 4), (5, 5), (6, 6)])


# ---- the plan and both passes on the host


@pytest.fixture(scope="module")
def host():
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    # a missing header or source fails here (getmtime, then the compiler): it is not a reason to skip
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        tmp = f"{OUT}.{os.getpid()}.tmp"  # pytest-xdist workers may build at once: write aside, rename
        subprocess.run([cxx, *FLAGS, "-fPIC", "-shared", "-o", tmp, SRC], check=True)
        os.replace(tmp, OUT)
    L = ctypes.CDLL(OUT)
    vp = ctypes.c_void_p
    L.tp_run.restype = ctypes.c_longlong
    L.tp_run.argtypes = [vp, ctypes.c_longlong, vp, vp, vp, vp, ctypes.c_int, ctypes.c_longlong, vp]
    L.tp_default_cap.restype = ctypes.c_longlong
    return L


def _walk(host, jobs, wms, preserve, cap):
    """Run the host walk into tiles carved out of one 0x5A buffer with gaps -> (tiles, info)."""
    sizes = np.array([(*wm, *t) for wm, t in jobs], np.int32)
    wm_all = np.concatenate([w.ravel() for w in wms])
    wm_off = np.cumsum([0] + [w.size for w in wms[:-1]]).astype(np.int64)
    gaps = [5 + 3 * i for i in range(len(jobs))]  # odd offsets: no tile starts aligned by accident
    tile_off, o = [], 0
    for g, (_, (th, tw)) in zip(gaps, jobs):
        o += g
        tile_off.append(o)
        o += th * tw
    buf = np.full(o + 11, 0x5A, np.uint8)
    info = np.zeros(4, np.int64)
    rc = host.tp_run(sizes.ctypes.data, len(jobs), wm_all.ctypes.data, wm_off.ctypes.data, buf.ctypes.data,
                     np.array(tile_off, np.int64).ctypes.data, int(preserve), cap, info.ctypes.data)
    assert rc == -1, rc
    written = np.zeros(buf.size, bool)
    tiles = []
    for off, (_, (th, tw)) in zip(tile_off, jobs):
        tiles.append(buf[off:off + th * tw].reshape(th, tw))
        written[off:off + th * tw] = True
    assert (buf[~written] == 0x5A).all(), "a byte outside the tiles was written"
    return tiles, [int(x) for x in info]


@pytest.mark.parametrize("preserve", [False, True])
def test_host_walk_matches_the_oracle(host, preserve):
    """List J through the plan and both grids on the host: every tile the oracle's, every gap byte
    untouched, one axis per distinct (in, out) pair; then with the scratch bound lowered to 8000
    bytes (the two 300 x 80 jobs alone exceed it) and to 1 byte (every job with a horizontal pass starts a group)."""
    assert host.tp_segment() in (64, 256) and host.tp_job_bytes() == 104
    assert host.tp_default_cap() == 64 << 20
    want = expected(preserve)
    tiles, (axes, groups, scratch, launches) = _walk(host, JOBS, list(watermarks()), preserve, host.tp_default_cap())
    for i, (t, w) in enumerate(zip(tiles, want)):
        assert np.array_equal(t, w), (preserve, i, JOBS[i])
    assert axes == distinct_axes(preserve), (axes, distinct_axes(preserve))
    assert groups == 1 and launches == 2 and scratch > 0
    assert not np.array_equal(tiles[2], tiles[3])  # one plan, two data sets
    need_h = sum(resized(wm, t, preserve)[1] != wm[1] for wm, t in JOBS)
    for cap, least in ((8000, 3), (1, need_h)):
        tiles_c, (axes_c, groups_c, scratch_c, launches_c) = _walk(host, JOBS, list(watermarks()), preserve, cap)
        print("cap", cap, "groups", groups_c, "scratch", scratch_c, "launches", launches_c)
        assert groups_c >= least and scratch_c < scratch and axes_c == axes
        assert groups_c < launches_c <= 2 * groups_c  # a group without a horizontal job launches once
        for i, (t, w) in enumerate(zip(tiles_c, want)):
            assert np.array_equal(t, w), (preserve, cap, i, JOBS[i])


def test_host_walk_refuses_the_error_jobs(host):
    for k, job in enumerate(ERROR_JOBS):
        jobs = [JOBS[4], job]
        sizes = np.array([(*wm, *t) for wm, t in jobs], np.int32)
        wm = np.zeros(29 * 31 + 700, np.uint8)
        buf = np.full(17 * 25 + 15, 0x5A, np.uint8)
        off = np.array([0, 29 * 31], np.int64)
        toff = np.array([0, 17 * 25], np.int64)
        info = np.zeros(4, np.int64)
        assert host.tp_run(sizes.ctypes.data, 2, wm.ctypes.data, off.ctypes.data, buf.ctypes.data, toff.ctypes.data, 1, 1 << 26,
                           info.ctypes.data) == 1
        assert (buf == 0x5A).all()


# ---- the pipeline's grouping with a fake device stage


class _FakeStage:
    """Marks pixel (0, 0) of every image with (watermark index, group, position in the group)."""

    def __init__(self):
        self.groups = []

    def __call__(self, rgbs, indices):
        g = len(self.groups)
        self.groups.append(list(indices))
        out = []
        for pos, (rgb, i) in enumerate(zip(rgbs, indices)):
            px = rgb.copy()
            px[0, 0] = (i, g, pos)
            out.append((px, None))
        return out


@pytest.mark.parametrize("k,groups", [(4, [[0, 1, 2, 3], [4, 5]]), (2, [[0, 1], [2, 3], [4, 5]])])
def test_pipeline_keeps_order_and_grouping(k, groups):
    sizes = [(48, 64), (40, 56), (64, 48), (48, 64), (40, 56), (64, 48)]
    imgs = [Image.fromarray(np.random.default_rng(40 + i).integers(0, 256, (h, w, 3), dtype=np.uint8)) for i, (h, w) in enumerate(sizes)]
    wms = [Image.fromarray(np.full((5, 5), 10 * i, np.uint8), "L") for i in range(6)]
    stage = _FakeStage()
    res = pipeline.embed_images(imgs, wms, True, {"block_size": 8}, workers=2, device_stage=stage, batch_images=k)
    assert stage.groups == groups
    for i, r in enumerate(res):
        ref = np.asarray(imgs[i]).copy()
        g = next(n for n, grp in enumerate(groups) if i in grp)
        assert tuple(r.pixels[0, 0]) == (i, g, groups[g].index(i))
        ref[0, 0] = r.pixels[0, 0]
        assert np.array_equal(r.pixels, ref), i
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(r.png))), ref), i
