// Device functions of the extract strip pass and of the edge pass, shared by the single-size
// kernels (tmfwm_kernels.hip) and the ragged ones (tmfwm_ragged_strip.hip, tmfwm_ragged.hip).
#pragma once
#include "tmfwm_blocks.h"

namespace tmf {

// ---------------------------------------------------------------------------
// Extract: watermarking.py:241-289 fused; sigma_1 of both images per block.
// ---------------------------------------------------------------------------
// f32 power iterations before certification: the strip pass certifies after 3
// (all but ~0.06 % of noise-cover blocks); the undecided go to the list pass, which certifies
// after 8, and what it still leaves undecided to the dgesdd route
constexpr int kPowerIters = 3;
constexpr int kListPowerIters = 8;
constexpr int kExtract8Waves = 3;  // waves per SIMD the register allocation of extract<b <= 8> allows

template <int B, int PX = 3>
TMF_DEVI void dct_rows_of(const uint32_t (&words)[Geo<B>::R][Geo<B, PX>::NW], int q, float *tile, float (&x)[Geo<B>::R][B])
{
    luma_rows<B, PX>(words, x);
    dct2d_rows_layout<B, false>(x, tile, q);
}

// sigma_1 of both images' blocks of this wave (pos per lane), certified or not (ok)
template <int B, int ITERS>
TMF_DEVI void extract_sigmas(const ExtractArgs &a, const StripPos &pos, float *tile, int q, float &sw, float &so, bool &ok)
{
    constexpr int R = Geo<B>::R, L = Geo<B>::L;
    if constexpr (B <= 14) {
        // both images' rows requested up front (one exposed HBM latency per wave, not two),
        // and both power iterations interleaved (sigma1_certified, NI = 2); at b = 16 the
        // interleaved form measured the same as the sequential one, at b = 14 -3 %
        // (profiles/r05/r05y_ab.log)
        float x[2][R][B];
        {
            uint32_t ww[R][Geo<B>::NW], wo[R][Geo<B>::NW];
            load_block_rows<B>(a.wsrc + pos.frame * a.frame_stride, a.W, pos, q, a.aligned, ww);
            load_block_rows<B>(a.osrc + pos.frame * a.frame_stride, a.W, pos, q, a.aligned, wo);
            dct_rows_of<B>(ww, q, tile, x[0]);
            dct_rows_of<B>(wo, q, tile, x[1]);
        }
        float s[2];
        bool k[2];
        sigma1_certified<B, L, ITERS, 2>(x, s, k);
        sw = s[0];
        so = s[1];
        ok = k[0] && k[1];
    } else {
        uint32_t w[R][Geo<B>::NW];
        float x[1][R][B], s[1];
        bool k[1];
        load_block_rows<B>(a.wsrc + pos.frame * a.frame_stride, a.W, pos, q, a.aligned, w);
        dct_rows_of<B>(w, q, tile, x[0]);
        sigma1_certified<B, L, ITERS, 1>(x, s, k);
        sw = s[0];
        ok = k[0];
        load_block_rows<B>(a.osrc + pos.frame * a.frame_stride, a.W, pos, q, a.aligned, w);
        dct_rows_of<B>(w, q, tile, x[0]);
        sigma1_certified<B, L, ITERS, 1>(x, s, k);
        so = s[0];
        ok = ok && k[0];
    }
}

// :285 under numpy-2 NEP 50: (f32 - f32) / f32(alpha) in f32; :288-289 clip, *255 in f64, trunc
TMF_DEVI uint8_t extract_byte(float sw, float so, float alpha32)
{
    const float e = (sw - so) / alpha32;
    double d = (double)e;
    d = d < 0.0 ? 0.0 : d;
    d = d > 1.0 ? 1.0 : d;
    return (uint8_t)(uint32_t)(d * 255.0);
}

// ---------------------------------------------------------------------------
// Pixels outside the full-block grid only get the colour round trip (:166, :216).
// ---------------------------------------------------------------------------
// the colour round trip of edge pixel idx (right strip first, then the bottom rows) of the frame at byte offset base
TMF_DEVI void edge_roundtrip_pixel(const EdgeArgs &a, int64_t idx, int64_t base)
{
    const int64_t right = (int64_t)a.core_h * a.edge_w;  // right strip: rows [0,core_h), cols [core_w, W)
    const int64_t bottom = (int64_t)(a.H - a.core_h) * a.W;
    if (idx >= right + bottom) return;
    int y, x;
    if (idx < right) {
        y = (int)(idx / a.edge_w);
        x = a.core_w + (int)(idx % a.edge_w);
    } else {
        const int64_t k = idx - right;
        y = a.core_h + (int)(k / a.W);
        x = (int)(k % a.W);
    }
    const int64_t off = base + ((int64_t)y * a.W + x) * 3;
    const uint32_t r = a.src[off], g = a.src[off + 1], b = a.src[off + 2];
    float cbs, crs;
    chroma(r, g, b, cbs, crs);
    uint32_t R8, G8, B8;
    colour_inv(luma(r, g, b), cbs, crs, R8, G8, B8);
    a.dst[off] = (uint8_t)R8;
    a.dst[off + 1] = (uint8_t)G8;
    a.dst[off + 2] = (uint8_t)B8;
}

}  // namespace tmf
