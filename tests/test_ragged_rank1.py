"""The ragged embed on the rank-1 routes, on the CPU: tmfwm_embed_ragged_rank1 and
tmfwm_embed_key_ragged_rank1 are exported and declared, check their arguments before any device
call and need a device for a valid call; the Python functions refuse an unsupported block first;
and the list pass's segment layout (tmfwm_ragged.h), built for the host from the header the
kernels use, partitions every chunk's list exactly.  No compute runs here."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from thatsmyface_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tmfwm_embed_ragged_rank1", "tmfwm_embed_key_ragged_rank1")


def test_symbols_exported_and_declared():
    L = _lib.load()
    for name in NAMES:
        assert hasattr(L, name), name
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == 8
    assert L.tmfwm_abi_version() == _lib.ABI_VERSION == 10  # new entry points within ABI 10


def _calls():
    """(embed, embed with key) callables over valid 16 x 16 descriptors, and the descriptor arrays."""
    L = _lib.load()
    a = np.zeros((16, 16, 3), np.uint8)
    o = np.empty_like(a)
    t = np.zeros((2, 2), np.uint8)
    k = np.zeros((2, 2), np.float32)
    keep = (a, o, t, k)
    ed = (_lib.EmbedFrame * 2)(*[_lib.EmbedFrame(a.ctypes.data, o.ctypes.data, t.ctypes.data, 16, 16) for _ in range(2)])
    kd = (_lib.EmbedKeyFrame * 2)(*[_lib.EmbedKeyFrame(a.ctypes.data, o.ctypes.data, t.ctypes.data, k.ctypes.data, 16, 16)
                                    for _ in range(2)])

    def make(fn, default):
        def call(block=8, alpha=0.1, mem=_lib.MEM_HOST, route=_lib.ROUTE_RANK1, n=2, desc=default, _k=keep):
            return fn(ctypes.addressof(desc) if desc is not None else None, n, block, alpha, mem, None, route, None)

        return call

    return make(L.tmfwm_embed_ragged_rank1, ed), make(L.tmfwm_embed_key_ragged_rank1, kd), ed, kd


def test_argument_validation_before_device():
    embed, embed_key, ed, kd = _calls()
    for call in (embed, embed_key):
        assert call(n=2, desc=None) == _lib.ERR_INVALID and "NULL" in _lib.last_error()  # NULL array with n > 0
        assert call(n=-1) == _lib.ERR_INVALID  # negative count
        for route in (_lib.ROUTE_HYBRID, _lib.ROUTE_REFERENCE, _lib.ROUTE_RANK1, _lib.ROUTE_RANK1_REFERENCE):
            for bad_block in (7, 18, 2):
                assert call(block=bad_block, route=route) == _lib.ERR_UNSUPPORTED
            assert call(route=route) in (0, _lib.ERR_NODEVICE), _lib.last_error()  # all four routes are accepted
        for bad_route in (-1, 4):
            assert call(route=bad_route) == _lib.ERR_INVALID and "route" in _lib.last_error()
        for bad_mem in (-1, 2):
            assert call(mem=bad_mem) == _lib.ERR_INVALID and "mem_kind" in _lib.last_error()
        assert call(alpha=float("nan")) == _lib.ERR_INVALID and "alpha" in _lib.last_error()
    # inside a descriptor: negative sizes and NULL pointers, in the second frame, for both memory kinds
    for mem in (_lib.MEM_HOST, _lib.MEM_DEVICE):
        for desc, call, fields in ((ed, embed, ("rgb", "out", "wm_tile")), (kd, embed_key, ("rgb", "out", "wm_tile", "out_key"))):
            for field in ("height", "width"):
                old = getattr(desc[1], field)
                setattr(desc[1], field, -3)
                assert call(mem=mem) == _lib.ERR_INVALID and "frame 1" in _lib.last_error(), (mem, field)
                setattr(desc[1], field, old)
            for field in fields:
                old = getattr(desc[1], field)
                setattr(desc[1], field, None)
                assert call(mem=mem) == _lib.ERR_INVALID and "NULL" in _lib.last_error(), (mem, field)
                setattr(desc[1], field, old)
    # a frame without a block needs no tile and no key; one of zero height needs no pointer at all
    for desc, call in ((ed, embed), (kd, embed_key)):
        desc[1].wm_tile, desc[1].height = None, 7
        if call is embed_key:
            desc[1].out_key = None
        assert call() in (0, _lib.ERR_NODEVICE), _lib.last_error()
        desc[1].rgb, desc[1].out, desc[1].height = None, None, 0
        assert call() in (0, _lib.ERR_NODEVICE), _lib.last_error()


def test_valid_call_needs_a_device():
    """Without a GPU a valid call fails with TMFWM_ERR_NODEVICE (no CPU fallback); with one it runs."""
    embed, embed_key, _, _ = _calls()
    if _lib.device_count() > 0:
        assert embed() == 0 and embed_key() == 0, _lib.last_error()
        return
    for call in (embed, embed_key):
        for mem in (_lib.MEM_HOST, _lib.MEM_DEVICE):
            for route in (_lib.ROUTE_RANK1, _lib.ROUTE_RANK1_REFERENCE):
                assert call(mem=mem, route=route) == _lib.ERR_NODEVICE and "no HIP device" in _lib.last_error()
        assert call(n=0, desc=None) == _lib.ERR_NODEVICE


def test_python_functions_refuse_block_first():
    batch = pytest.importorskip("thatsmyface_amd.batch")
    for fn in (batch.embed_ragged_rank1, batch.embed_with_key_ragged_rank1):
        for route in ("rank1", "rank1_reference", "hybrid"):
            with pytest.raises(NotImplementedError, match="block 7"):
                fn([object()], [object()], 7, 0.1, route=route)  # no tensor is looked at
        with pytest.raises(ValueError):
            fn([], [], 8, 0.1, route="rank2")


# ---- the list pass's segment layout

SRC = os.path.join(ROOT, "tests", "native", "ragged_shard_host.cpp")
HDRS = [os.path.join(ROOT, "thatsmyface_amd", "csrc", h) for h in ("tmfwm_ragged.h", "tmfwm_internal.h")]
OUT = os.path.join(ROOT, "tests", "_build", "libragged_shard_host.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def shard_lib():
    if not os.path.exists(HIPCC) and not shutil.which("hipcc"):
        pytest.skip("hipcc not available")
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(p) for p in [SRC] + HDRS):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        tmp = f"{OUT}.{os.getpid()}.tmp"
        subprocess.run([HIPCC, "-O2", "-std=c++17", "-fPIC", "-x", "hip", "--offload-arch=gfx950", "-shared", "-o", tmp, SRC],
                       check=True)
        os.replace(tmp, OUT)
    L = ctypes.CDLL(OUT)
    L.ragged_shard_check.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p]
    L.ragged_shard_count.restype = ctypes.c_uint32
    return L


def _check(lib, frames, cap=1 << 29):
    """frames: (nbh, nbw) per frame -> the number of chunks; asserts every chunk's segments partition its list."""
    nbh = np.array([f[0] for f in frames], np.int32)
    nbw = np.array([f[1] for f in frames], np.int32)
    n = ctypes.c_int64(-1)
    rc = lib.ragged_shard_check(nbh.ctypes.data, nbw.ctypes.data, len(frames), cap, ctypes.addressof(n))
    assert rc == 0, (rc, frames[:8], cap)
    return n.value


def test_segments_partition_every_chunk(shard_lib):
    K = shard_lib.ragged_shard_count()
    assert K == 2048
    rng = np.random.default_rng(7)
    # one frame: one row, fewer rows than shards, as many, more; a 4K frame at b = 4 (540 x 960 blocks)
    for nbh in (1, 2, 17, K - 1, K, K + 1, 3 * K + 5):
        for nbw in (1, 3, 240):
            assert _check(shard_lib, [(nbh, nbw)]) == 1
    assert _check(shard_lib, [(540, 960)]) == 1
    assert _check(shard_lib, [(540, 960)] * 5 + [(3, 4)] + [(540, 960)] * 3) == 1  # the small frame keeps a shard
    # frames with fewer rows than their share of the shards, and frames without a block between frames with blocks
    assert _check(shard_lib, [(1, 5), (2, 3), (1, 1)]) == 1
    assert _check(shard_lib, [(0, 7), (3, 5), (0, 0), (4, 0), (2, 9), (0, 3), (5, 1), (0, 2)]) == 1
    mixed = [(int(rng.integers(0, 4)), int(rng.integers(0, 6))) for _ in range(70)]
    assert _check(shard_lib, mixed) == 1
    # the block cap cuts chunks (ids and shard ranges are relative to the chunk)
    assert _check(shard_lib, mixed, cap=40) >= 3
    # more frames with blocks than shards: the chunk splits, frames without a block do not count
    assert _check(shard_lib, [(1, 1)] * K) == 1
    assert _check(shard_lib, [(1, 1)] * (K + 1)) == 2
    assert _check(shard_lib, [(2, 3), (0, 5)] * K + [(7, 2)]) == 2
    assert _check(shard_lib, [(int(rng.integers(1, 9)), int(rng.integers(1, 9))) for _ in range(2 * K + 3)]) == 3
