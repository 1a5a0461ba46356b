"""Altered uploads for the extract tests -- test infrastructure only.

A verifier extracts from images it did not produce: an embed output that has been recompressed,
brightened, blurred, resized, shifted, or swapped for another picture.  The generators here make
such uploads from an embed output `w` and its cover `c`, seeded, with numpy and Pillow's filters
only (no codec: `jpegish` restates JPEG's 8 x 8 YCbCr DCT quantisation in numpy).  Every class is
an (upload, original) pair of RGB u8 frames of one size.

The embed is always at alpha 0.1; the alpha of the EXTRACT call is what the tests vary
(EXTRACT_ALPHAS), because the quotient (sigma_w - sigma_o) / alpha of an altered upload is not the
watermark byte any more: a shift or a brightness change moves sigma_1 by more than 0.1, and only a
larger alpha brings the quotient back inside (0, 1), where a wrong sigma_1 shows in the byte.

The module also holds the sigma_1 enclosure model's block counts for such pairs (model_counts):
what the widened list-pass model and the strip-pass model (tests/sigma1_helpers.py) leave
undecided in EITHER image of a pair, the bounds the GPU's `lapack_blocks` and `list_pass_blocks`
are held to."""
from __future__ import annotations

import functools
import os
import sys

import numpy as np
from PIL import Image, ImageFilter

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sigma1_helpers as S  # noqa: E402
from keyed_helpers import bytes_of, sparks  # noqa: E402
from lapack_path import photo_cover  # noqa: E402

from oracle import oracle as O  # noqa: E402

BLOCKS = (4, 6, 8, 10, 12, 14, 16)
EMBED_ALPHA = 0.1
THREADS = min(8, O.default_threads())  # the frames hold some 420 blocks: more threads cost more to start than they save
CLIPPING = ("same", "other", "flip", "swapped")  # kept although their bytes clip at every alpha
JPEGISH_QUALITIES = (90, 60)

# ITU-T T.81 Annex K tables 1 and 2 (the standard luminance / chrominance quantisers)
_LUMA_Q = np.array([
    [16, 11, 10, 16, 24, 40, 51, 61], [12, 12, 14, 19, 26, 58, 60, 55], [14, 13, 16, 24, 40, 57, 69, 56],
    [14, 17, 22, 29, 51, 87, 80, 62], [18, 22, 37, 56, 68, 109, 103, 77], [24, 35, 55, 64, 81, 104, 113, 92],
    [49, 64, 78, 87, 103, 121, 120, 101], [72, 92, 95, 98, 112, 100, 103, 99]], np.float64)
_CHROMA_Q = np.array([
    [17, 18, 24, 47, 99, 99, 99, 99], [18, 21, 26, 66, 99, 99, 99, 99], [24, 26, 56, 99, 99, 99, 99, 99],
    [47, 66, 99, 99, 99, 99, 99, 99], [99, 99, 99, 99, 99, 99, 99, 99], [99, 99, 99, 99, 99, 99, 99, 99],
    [99, 99, 99, 99, 99, 99, 99, 99], [99, 99, 99, 99, 99, 99, 99, 99]], np.float64)
_k = np.arange(8)
_C8 = np.sqrt(2.0 / 8.0) * np.cos((2 * _k[None, :] + 1) * _k[:, None] * np.pi / 16.0)  # orthonormal DCT-II, rows = frequencies
_C8[0] /= np.sqrt(2.0)


def _quant_table(base: np.ndarray, quality: int) -> np.ndarray:
    """The table scaled the way the IJG library scales it for a quality of 1..100."""
    scale = 5000.0 / quality if quality < 50 else 200.0 - 2.0 * quality
    return np.clip(np.floor((base * scale + 50.0) / 100.0), 1.0, 255.0)


def jpegish(rgb: np.ndarray, quality: int) -> np.ndarray:
    """JPEG-shaped loss without a codec: full-range BT.601 YCbCr, per plane an 8 x 8 orthonormal
    DCT of the level-shifted samples (edges replicated up to a multiple of 8), coefficients rounded
    to multiples of the scaled standard tables, and back.  No chroma subsampling, no entropy coding."""
    rgb = np.ascontiguousarray(rgb, np.uint8)
    H, W = rgb.shape[:2]
    x = rgb.astype(np.float64)
    r, g, b = x[..., 0], x[..., 1], x[..., 2]
    planes = [0.299 * r + 0.587 * g + 0.114 * b,
              128.0 - 0.168736 * r - 0.331264 * g + 0.5 * b,
              128.0 + 0.5 * r - 0.418688 * g - 0.081312 * b]
    Hp, Wp = -(-H // 8) * 8, -(-W // 8) * 8
    out = []
    for p, base in zip(planes, (_LUMA_Q, _CHROMA_Q, _CHROMA_Q)):
        q = _quant_table(base, quality)
        p = np.pad(p, ((0, Hp - H), (0, Wp - W)), mode="edge") - 128.0
        blk = p.reshape(Hp // 8, 8, Wp // 8, 8).transpose(0, 2, 1, 3)
        coef = np.einsum("ux,ijxy,vy->ijuv", _C8, blk, _C8)
        coef = np.round(coef / q) * q
        blk = np.einsum("ux,ijuv,vy->ijxy", _C8, coef, _C8)
        out.append(blk.transpose(0, 2, 1, 3).reshape(Hp, Wp)[:H, :W] + 128.0)
    y, cb, cr = out[0], out[1] - 128.0, out[2] - 128.0
    back = np.stack([y + 1.402 * cr, y - 0.344136 * cb - 0.714136 * cr, y + 1.772 * cb], -1)
    return np.clip(np.round(back), 0, 255).astype(np.uint8)


def noise3(w: np.ndarray, seed: int) -> np.ndarray:
    n = np.random.default_rng(seed).integers(-3, 4, w.shape)
    return np.clip(w.astype(np.int64) + n, 0, 255).astype(np.uint8)


def plus2(w: np.ndarray) -> np.ndarray:
    return np.clip(w.astype(np.int64) + 2, 0, 255).astype(np.uint8)


def gamma(w: np.ndarray, g: float = 0.97) -> np.ndarray:
    lut = np.round(255.0 * (np.arange(256) / 255.0) ** g).astype(np.uint8)
    return lut[w]


def blur(w: np.ndarray, radius: float = 0.6) -> np.ndarray:
    return np.asarray(Image.fromarray(w, "RGB").filter(ImageFilter.GaussianBlur(radius)))


def resize(w: np.ndarray) -> np.ndarray:
    H, W = w.shape[:2]
    small = Image.fromarray(w, "RGB").resize((max(1, 3 * W // 4), max(1, 3 * H // 4)), Image.BILINEAR)
    return np.asarray(small.resize((W, H), Image.BICUBIC))


def shift(w: np.ndarray) -> np.ndarray:
    return np.roll(w, (1, 2), axis=(0, 1))


def flip(w: np.ndarray) -> np.ndarray:
    return w[:, ::-1]


def drop2bits(w: np.ndarray) -> np.ndarray:
    return (w & 0xFC) | 2


def other(w: np.ndarray, seed: int) -> np.ndarray:
    return photo_cover(w.shape[0], w.shape[1], seed + 7919)


def uploads(w: np.ndarray, c: np.ndarray, seed: int) -> dict:
    """name -> (upload, original), contiguous RGB u8 frames of w's size, in a fixed order."""
    w, c = np.ascontiguousarray(w, np.uint8), np.ascontiguousarray(c, np.uint8)
    assert w.shape == c.shape and w.ndim == 3 and w.shape[2] == 3
    made = {f"jpegish{q}": jpegish(w, q) for q in JPEGISH_QUALITIES}
    made.update(noise3=noise3(w, seed), plus2=plus2(w), gamma=gamma(w), blur=blur(w), resize=resize(w), shift=shift(w),
                flip=flip(w), drop2bits=drop2bits(w), other=other(w, seed), same=c)
    pairs = {k: (np.ascontiguousarray(v, np.uint8), c) for k, v in made.items()}
    pairs["swapped"] = (c, w)
    return pairs


def key_of(rgb: np.ndarray, b: int) -> np.ndarray:
    """keyed_helpers.key_of (the oracle's dgesdd-route f32 sigma_1 per block) on THREADS threads."""
    nbh, nbw = rgb.shape[0] // b, rgb.shape[1] // b
    return np.ascontiguousarray(O.lp_svd_blocks(S.frame_blocks(rgb, b), nthreads=THREADS)[1][:, 0].reshape(nbh, nbw))


def expect(up: np.ndarray, orig: np.ndarray, b: int, alpha: float) -> np.ndarray:
    """The oracle's dgesdd-route bytes of one pair."""
    return O.extract_frame(up, orig, b, alpha, nthreads=THREADS, route="lapack")


# ------------------------------------------------------------------ the frames the tests share
def cover(kind: str, H: int, W: int, seed: int) -> np.ndarray:
    if kind == "photo":
        return photo_cover(H, W, seed)
    from golden.gen_golden import cover as golden_cover

    return np.ascontiguousarray(golden_cover(kind, H, W, seed))  # "noise", "qr"


def frame_size(b: int):
    """6 x 70 blocks (6 x 71 at b = 4) with partial strips and edge pixels on both axes."""
    return 6 * b + 3, 70 * b + 5


class Corpus:
    """One cover of frame_size(b), its embed output at alpha 0.1 with a noise tile, and every
    class of it: names, the stacked uploads and originals (n, H, W, 3), and what the oracle's
    dgesdd route makes of them.  Built once per (b, cover kind) and never written to."""

    def __init__(self, b: int, kind: str):
        self.b, self.kind = b, kind
        H, W = frame_size(b)
        seed = 1000 * b + {"photo": 1, "noise": 2, "qr": 3}[kind]
        self.cover = cover(kind, H, W, seed)
        self.tile = np.random.default_rng(seed + 50).integers(0, 256, (H // b, W // b), dtype=np.uint8)
        self.embed = O.embed_frame(self.cover, self.tile, b, EMBED_ALPHA, nthreads=THREADS)
        pairs = uploads(self.embed, self.cover, seed)
        self.names = tuple(pairs)
        self.up = np.stack([pairs[k][0] for k in self.names])
        self.orig = np.stack([pairs[k][1] for k in self.names])
        for a in (self.cover, self.tile, self.embed, self.up, self.orig):
            a.setflags(write=False)
        self._expect = {}

    @functools.cached_property
    def keys_up(self) -> np.ndarray:
        """(n, nbh, nbw) f32: the oracle's dgesdd-route key of every upload."""
        return np.stack([key_of(f, self.b) for f in self.up])

    @functools.cached_property
    def keys_orig(self) -> np.ndarray:
        by_id = {}
        return np.stack([by_id.setdefault(f.tobytes(), key_of(f, self.b)) for f in self.orig])

    def expect(self, alpha: float) -> np.ndarray:
        """(n, nbh, nbw) u8: O.extract_frame(upload, original, b, alpha, route="lapack") per class."""
        if alpha not in self._expect:
            self._expect[alpha] = np.stack([expect(u, o, self.b, alpha) for u, o in zip(self.up, self.orig)])
        return self._expect[alpha]

    @functools.cached_property
    def counts(self) -> dict:
        return model_counts(self.up, self.orig, self.b)


@functools.lru_cache(maxsize=None)
def corpus(b: int, kind: str) -> Corpus:
    return Corpus(b, kind)


def extract_alphas(b: int):
    """The alphas of the extract calls.  0.25 is there for `plus2` at b = 16: +2 levels move sigma_1 by
    2 b / 255 = 0.125, and the bytes of (0.125 .. 0.225) / alpha are all inside (0, 255) at 0.5 but
    take only 30 distinct values there; at 0.25 they take about 60."""
    return (0.1, 0.25, 0.5, 2.0, float(b))


def informative(tile_bytes: np.ndarray) -> bool:
    """At least a quarter of the bytes strictly between the clip values, and 32 distinct values."""
    t = np.asarray(tile_bytes).ravel()
    return bool(((t >= 1) & (t <= 254)).mean() >= 0.25 and len(np.unique(t)) >= 32)


def interior_share(tile_bytes: np.ndarray) -> float:
    t = np.asarray(tile_bytes).ravel()
    return float(((t >= 1) & (t <= 254)).mean())


# ------------------------------------------------------------------ the enclosure model's counts
def undecided(rgb: np.ndarray, b: int, iters: int, widen: float = 1.0) -> np.ndarray:
    """(nbh, nbw) bool: the blocks of a frame whose sigma_1 the model's enclosure, scaled by `widen`
    about its centre, does not decide after `iters` power steps."""
    nbh, nbw = rgb.shape[0] // b, rgb.shape[1] // b
    return ~S.enclosure(S.frame_blocks(rgb, b), iters, widen=widen)[2].reshape(nbh, nbw)


def never_decided(rgb: np.ndarray, b: int) -> np.ndarray:
    """(nbh, nbw) bool: blocks with F > 0 and 2 sigma_1^2 <= F (1 - 2^-40) by LAPACK's own sigma_1.
    rho <= sigma_1^2 (1 + a few u) for any vector, so 2 rho > F fails whatever the kernel iterates."""
    D = S.frame_blocks(rgb, b)
    F = np.sum(D.astype(np.float64) ** 2, axis=(1, 2))
    s = S.sigma1_lapack(D)
    return ((F > 0.0) & (2.0 * s * s <= F * (1.0 - 2.0 ** -40))).reshape(rgb.shape[0] // b, rgb.shape[1] // b)


def model_counts(ups, origs, b: int) -> dict:
    """Per-pair masks over the block grid, True where EITHER image's block is concerned:
      "list"   undecided by the model widened by KEEP_WIDEN after the list pass's iterations --
               the most a hybrid call with a list pass may send to the dgesdd route;
      "strip"  undecided by the model after the strip pass's iterations -- the most the strip
               pass may hand on (to the list pass, or on the ragged calls to the dgesdd route);
      "never"  2 sigma_1^2 <= F: no vector decides, the least the dgesdd route gets.
    Frames that repeat (one original under many uploads) are modelled once."""
    memo = {}

    def masks(f):
        k = f.tobytes()
        if k not in memo:
            memo[k] = (undecided(f, b, S.LIST_ITERS, S.KEEP_WIDEN), undecided(f, b, S.strip_iters(b)), never_decided(f, b))
        return memo[k]

    out = {"list": [], "strip": [], "never": []}
    for u, o in zip(ups, origs):
        mu, mo = masks(np.ascontiguousarray(u)), masks(np.ascontiguousarray(o))
        for name, a, c in zip(("list", "strip", "never"), mu, mo):
            out[name].append(a | c)
    return {k: np.stack(v) if v else np.zeros((0, 0, 0), bool) for k, v in out.items()}


# ------------------------------------------------------------------ one side undecided
def sparks_pairs(b: int) -> dict:
    """Four (upload, original, sparks mask) arrangements of frame_size(b) in which the dgesdd route
    is forced for one image of a pair while the other holds an ordinary photo block:
      "orig_sparks"  original all sparks, upload a photo;
      "up_sparks"    the reverse;
      "orig_cols"    original a photo with sparks in block columns 17 onward, upload the photo's embed output;
      "ell"          that original, and the upload with sparks in the lower half of the block rows:
                     the union of the two is an L.
    The mask is True where either image holds a sparks block."""
    H, W = frame_size(b)
    nbh, nbw = H // b, W // b
    cp = corpus(b, "photo")
    sp_o, sp_u = sparks(H, W, b, 77 + b), sparks(H, W, b, 177 + b)
    cols = np.zeros((nbh, nbw), bool)
    cols[:, 17:] = True
    rows = np.zeros((nbh, nbw), bool)
    rows[nbh // 2:] = True

    def paste(photo, sp, mask):
        px = np.kron(mask, np.ones((b, b), bool))
        out = photo.copy()
        out[: nbh * b, : nbw * b][px] = sp[: nbh * b, : nbw * b][px]
        return out

    full = np.ones((nbh, nbw), bool)
    o_cols = paste(cp.cover, sp_o, cols)
    return {"orig_sparks": (cp.embed, sp_o, full), "up_sparks": (sp_u, cp.cover, full),
            "orig_cols": (cp.embed, o_cols, cols), "ell": (paste(cp.embed, sp_u, rows), o_cols, cols | rows)}


def sparks_alphas(b: int):
    """float(b) brings photo-minus-sparks quotients inside (0, 1) at every size.  The sparks-minus-photo
    pair clips at float(b) (negative) and at -0.5 ((sigma_photo - 1) / 0.5 > 1 for nearly every block,
    share 0.10 at b = 4 and 0.00 above); -float(b) brings all of its bytes inside."""
    return (float(b), -0.5, -float(b))
