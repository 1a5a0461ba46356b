// Keyed extraction: device functions shared by the strip / list passes
// (tmfwm_keyed.hip), the dgesdd-route passes (tmfwm_keyed_fixup.hip) and the ragged keyed
// kernels (tmfwm_ragged_strip.hip, tmfwm_ragged_fixup.hip), which run them on one-frame views.
//
// extract's byte depends on the original image only through f32(sigma_1) of each of its blocks.
// sigma1_map stores that float per block -- the key -- and extract_keyed takes the key in place
// of the original's pixels.  Both run the pair path's arithmetic on one image: the certified
// enclosure (sigma1_certified) where it decides, the dgesdd route where it does not, so a key
// entry is np.linalg.svd's f32 S[0] on every route.
#pragma once
#include "tmfwm_fixup.h"
#include "tmfwm_passes.h"

namespace tmf {

// extract_byte against a stored key entry.  A key that is not finite (a damaged file) gives
// byte 0, and so does a quotient that is not >= 0: extract_byte's clip gives 0 for every
// negative quotient, and a NaN must not reach its integer cast.
TMF_DEVI uint8_t keyed_byte(float sw, float key, float alpha32)
{
    const float e = (sw - key) / alpha32;
    if (!(__builtin_fabsf(key) <= 3.4028234663852886e38f) || !(e >= 0.0f)) return 0;
    return extract_byte(sw, key, alpha32);
}

// this block's result: its key entry (MAP), or its byte against the stored entry
template <bool MAP>
TMF_DEVI void keyed_store(const KeyedArgs &a, int64_t frame, int bi, int bj, float s)
{
    const int64_t at = (int64_t)bi * a.nbw + bj;
    if constexpr (MAP) a.key_out[frame * a.key_stride + at] = s;
    else a.out[frame * a.tile_stride + at] = keyed_byte(s, a.key[frame * a.key_stride + at], a.alpha32);
}

// waves per SIMD the register allocation must allow: one image's rows and one power iteration
// live at a time, so the pair kernels' bounds hold with room to spare
template <int B>
constexpr int kKeyedWaves = B > 8 ? 2 : kExtract8Waves;

// sigma_1 of this wave's blocks of the one image (pos per lane), certified or not (ok).  PX: the
// frames' bytes per pixel (Geo<B, PX>); at PX = 4 a.aligned says that the frame base and the frame
// stride are multiples of 4 -- every block row is then whole aligned dwords, whatever W is
template <int B, int ITERS, int PX = 3>
TMF_DEVI void keyed_sigma(const KeyedArgs &a, const StripPos &pos, float *tile, int q, float &s, bool &ok)
{
    constexpr int R = Geo<B>::R, L = Geo<B>::L;
    uint32_t w[R][Geo<B, PX>::NW];
    float x[1][R][B], s1[1];
    bool k[1];
    load_block_rows<B, PX>(a.src + pos.frame * a.frame_stride, a.W, pos, q, a.aligned, w);
    dct_rows_of<B, PX>(w, q, tile, x[0]);
    sigma1_certified<B, L, ITERS, 1>(x, s1, k);
    s = s1[0];
    ok = k[0];
}

// a listed block on the dgesdd route: S[0] of np.linalg.svd's arithmetic, stored as keyed_store has it
template <int B, class Par, int G, bool MAP, int PX = 3>
TMF_DEVI void keyed_fix_block(const KeyedArgs &a, uint32_t id, FixLdsS<B> &f, int gl)
{
    const uint32_t per_frame = (uint32_t)a.nbh * (uint32_t)a.nbw;
    int64_t fr;
    int bi, bj;
    block_of(id, per_frame, a.nbw, fr, bi, bj);
    fix_load_dct<B, G, PX>(a.src + fr * a.frame_stride, a.W, bi, bj, f.D, gl);
    const int info = lp::svd_f32_ws<false, Par>(f.D, runtime_n(B), nullptr, f.S, nullptr, f.ws);  // :279-282
    if (info && gl == 0 && a.fb_bad) atomicAdd(a.fb_bad, 1u);
    const float s = f.S[0];
    group_sync();  // the LDS slots are reused by the next listed block
    if (gl == 0) keyed_store<MAP>(a, fr, bi, bj, s);
}

}  // namespace tmf
