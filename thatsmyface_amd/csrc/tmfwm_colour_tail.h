// The per-pixel colour tail of the embed kernels: source bytes + the Y interval -> output bytes
// and the pixel's share of the block's "undecided" flag (watermarking.py:207-216).
//
// The exact tail (chroma + colour_inv_frac + the wide test, tmfwm_device.h) evaluates the 3x3
// colour transforms in f64 only to truncate the result to a byte.  colour_tail_fast() decides
// the same bytes in f32 wherever the scaled channel values are provably away from a byte
// boundary; the remaining pixels (a few in 10^4) take the exact tail, so every byte and every
// undecided flag is what the exact tail alone gives.
//
// The fast path compiles for the host as well (tests/native/colour_tail_host.cpp): no HIP
// dependency off device, every fma written out (the TUs are built with -ffp-contract=off).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define TMF_CT_FN __host__ __device__ __forceinline__
#else
#define TMF_CT_FN inline
#endif

namespace tmf {
namespace ct {

// q = 255 Y + a . (R, G, B): the inverse rows applied to the forward chroma rows, the 1/255 of the
// bytes and the * 255 of the output folded into f32 coefficients (products of the f64 constants
// of tmfwm_device.h, rounded once):
//   R: 1.403 cr            G: -0.714 cr - 0.344 cb            B: 1.773 cb
//   cb = -0.169 R - 0.331 G + 0.5 B      cr = 0.5 R - 0.419 G - 0.081 B
constexpr float kRr = (float)(1.403 * 0.5), kRg = (float)(1.403 * -0.419), kRb = (float)(1.403 * -0.081);
constexpr float kGr = (float)(-0.714 * 0.5 - 0.344 * -0.169), kGg = (float)(-0.714 * -0.419 - 0.344 * -0.331),
                kGb = (float)(-0.714 * -0.081 - 0.344 * 0.5);
constexpr float kBr = (float)(1.773 * -0.169), kBg = (float)(1.773 * -0.331), kBb = (float)(1.773 * 0.5);

// |q - 255 v| + 2^-17 <= kDelta for every byte triple and every Y with |q| <= 256, v the exact
// tail's f32 channel value before the clip (DESIGN.md 3.5 derives 6.65 * 2^-16 for the worst
// channel, B); outside |q| <= 256 the error stays below |q| 2^-21 + kDelta.
constexpr float kDelta = 7.0f * 0x1p-16f;
// q is clamped to [kDelta, 255 + kDelta]: a channel at or beyond an end of it is clipped in the
// exact tail too (v <= 0 or v >= 1), and the end itself passes the lower test below
constexpr float kLo = kDelta, kHi = 255.0f + kDelta;
// upper test's constant: kDelta, the 2^-14 of the exact tail's bound on p(Yh) - p(Yl) and 2^-20
// for the f32 roundings of the test itself
constexpr float kUp = kDelta + 0x1p-14f + 0x1p-20f;

TMF_CT_FN float med3(float x, float lo, float hi)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_fmed3f(x, lo, hi);
#else
    x = x > lo ? x : lo;  // a NaN gives lo (the pixel is rejected by its dy)
    return x < hi ? x : hi;
#endif
}

TMF_CT_FN float fract(float x)  // x in [kLo, kHi]: exact
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_fractf(x);
#else
    return x - (float)(uint32_t)x;
#endif
}

}  // namespace ct

// The f32 decision.  Returns true when the pixel is accepted: R, G, B are then the exact tail's
// bytes at Y = yl and at every Y up to yl + |dy| (the upper end's bytes among them), so the pixel
// leaves its block decided.  With n = floor(q clamped) and f = q - n, per channel:
//   lower: f >= kDelta  =>  255 v >= n, so p(yl) = f32(clip(v) 255) >= n
//   upper: f + kDelta + 255.1 |dy| + 2^-14 < 1  =>  p(yl) + 255.1 |dy| + 2^-14 < n + 1, and the
//          exact tail's own argument puts p(yh) below the left side
// (a clipped channel sits on an end of the clamp, where f = kDelta: it passes the lower test by
// itself and the upper one unless dy is wide).  A non-finite yl or dy is rejected: dy = yh - yl
// is then non-finite, and so is the upper test's left side.
TMF_CT_FN bool colour_tail_fast(uint32_t R0, uint32_t G0, uint32_t B0, float yl, float dy, uint32_t &R, uint32_t &G, uint32_t &B)
{
    using namespace ct;
    const float r = (float)R0, g = (float)G0, b = (float)B0;
    const float qr = __builtin_fmaf(255.0f, yl, __builtin_fmaf(kRr, r, __builtin_fmaf(kRg, g, kRb * b)));
    const float qg = __builtin_fmaf(255.0f, yl, __builtin_fmaf(kGr, r, __builtin_fmaf(kGg, g, kGb * b)));
    const float qb = __builtin_fmaf(255.0f, yl, __builtin_fmaf(kBr, r, __builtin_fmaf(kBg, g, kBb * b)));
    const float cr = med3(qr, kLo, kHi), cg = med3(qg, kLo, kHi), cb = med3(qb, kLo, kHi);
    R = (uint32_t)cr;
    G = (uint32_t)cg;
    B = (uint32_t)cb;
    const float fr = fract(cr), fg = fract(cg), fb = fract(cb);
    const float lo = __builtin_fminf(fr, __builtin_fminf(fg, fb)), hi = __builtin_fmaxf(fr, __builtin_fmaxf(fg, fb));
    const float t = __builtin_fmaf(__builtin_fabsf(dy), 255.1f, kUp);
    return lo >= kDelta && hi + t < 1.0f;
}

#if defined(TMF_DEVI)  // after tmfwm_device.h: the colour tail of one pixel row of the embed kernels
#if defined(TMF_STAMPS) && defined(TMF_TAIL_COUNT)
// opt-in count (-DTMF_STAMPS -DTMF_TAIL_COUNT, tools/phase_stamps.py) in the phase stamps' spare
// slots, over the sampled waves: [12] pixel rows, [13] rows with a rejecting lane, [14] pixel
// steps, [15] pixel steps that ran the exact tail
extern __device__ unsigned long long g_stamps[16];
TMF_DEVI void tail_count(int slot, unsigned long long n)
{
    if ((threadIdx.x & 63) == 0 && (blockIdx.x & 63) == 0) atomicAdd(&g_stamps[slot], n);
}
#else
TMF_DEVI void tail_count(int, unsigned long long) {}
#endif

// The exact tail of one pixel: colour_inv_frac at yl, and colour_inv at yh only where the bytes
// could differ; `unc` collects the pixels whose ends give other bytes.
TMF_DEVI void colour_tail_exact(uint32_t R0, uint32_t G0, uint32_t B0, float yl, float yh, float dy, uint32_t &R8, uint32_t &G8,
                                uint32_t &B8, bool &unc)
{
    float cbs, crs, fr;
    chroma(R0, G0, B0, cbs, crs);
    colour_inv_frac(yl, cbs, crs, R8, G8, B8, fr);
    // Every channel is monotone in Y, and from Y's lower end to its upper end each scaled value
    // p = f32(clip(v) * 255) grows by at most 255 dY + 255 * 2^-24 + 2^-16 (v's f32 rounding on
    // [0, 1], then p's) < 255.1 dY + 2^-14; so the bytes cannot differ unless frac(p) + that
    // reaches 1, and only then are the upper end's bytes computed
    const bool wide = dy != 0.0f && fr + __builtin_fmaf(dy, 255.1f, 0x1p-14f) >= 1.0f;
    if (__builtin_amdgcn_ballot_w64(wide) != 0 && wide) {
        uint32_t R9, G9, B9;
        colour_inv(yh, cbs, crs, R9, G9, B9);
        unc = unc || R9 != R8 || G9 != G8 || B9 != B8;
    }
}

struct TailY {
    float yl, yh, dy;  // Y's lower and upper end, and the width the exact tail's wide test takes
};

TMF_DEVI uint32_t tail_byte(const uint32_t *w, int k) { return (w[k >> 2] >> (8 * (k & 3))) & 0xFFu; }

// Byte k of a row of packed words: into zeroed words (or), over earlier bytes (set)
template <bool SET>
TMF_DEVI void tail_put(uint32_t *w, int k, uint32_t v)
{
    const int sh = 8 * (k & 3);
    if constexpr (SET) w[k >> 2] = (w[k >> 2] & ~(0xFFu << sh)) | (v << sh);
    else w[k >> 2] |= v << sh;
}

// One row of B pixels: source bytes in `words`, y(c) the TailY of pixel c, output bytes packed
// into `out` (NW words).  The f32 decision runs over the whole row first, straight-line (the row's pixels are independent, and a
// branch per pixel would serialise the wave on each pixel's dependency chain); each lane records
// its rejected pixels in a bit mask, and only if some lane of the wave has one (a third of the
// rows on noise covers) the row is walked again and the rejected pixels take the exact tail, whose
// bytes replace the f32 path's.
// `hot` is wave-uniform state across the wave's rows (false before the first): a block that the
// watermark leaves alone (tile value 0) reproduces its own Y, and a grey or white pixel of it
// comes back on the byte boundary itself (each inverse row applied to the forward rows sums to
// 1), so flat grey content rejects everywhere.  Eight lanes rejecting in one row mark such content
// (independent rejections: ~7 * 10^-3 per lane and row); from then on the wave skips the f32
// decision and costs what the exact tail alone costs.
template <int B, class Y>
TMF_DEVI void colour_tail_row(const uint32_t *words, Y y, uint32_t *out, bool &unc, bool &hot)
{
    constexpr int NW = (3 * B + 3) / 4;
#pragma unroll
    for (int i = 0; i < NW; ++i) out[i] = 0u;
    uint32_t rej = ~0u;  // this lane's pixels left to the exact tail
    if (!hot) {
        rej = 0u;
#pragma unroll
        for (int c = 0; c < B; ++c) {
            const TailY t = y(c);
            uint32_t R8, G8, B8;
            const bool ok = colour_tail_fast(tail_byte(words, 3 * c), tail_byte(words, 3 * c + 1), tail_byte(words, 3 * c + 2),
                                             t.yl, t.dy, R8, G8, B8);
            rej |= ok ? 0u : 1u << c;
            tail_put<false>(out, 3 * c, R8);
            tail_put<false>(out, 3 * c + 1, G8);
            tail_put<false>(out, 3 * c + 2, B8);
        }
        const unsigned long long m = __builtin_amdgcn_ballot_w64(rej != 0u);
        tail_count(12, 1);
        tail_count(14, B);
        if (m == 0) return;
        tail_count(13, 1);
        hot = __builtin_popcountll(m) >= 8;
    } else {
        tail_count(12, 1);
        tail_count(13, 1);
        tail_count(14, B);
    }
#pragma unroll
    for (int c = 0; c < B; ++c) {
        const bool redo = (rej >> c) & 1u;
        if (__builtin_amdgcn_ballot_w64(redo) != 0) {
            tail_count(15, 1);
            if (redo) {
                const TailY t = y(c);
                uint32_t R8, G8, B8;
                colour_tail_exact(tail_byte(words, 3 * c), tail_byte(words, 3 * c + 1), tail_byte(words, 3 * c + 2), t.yl, t.yh,
                                  t.dy, R8, G8, B8, unc);
                tail_put<true>(out, 3 * c, R8);
                tail_put<true>(out, 3 * c + 1, G8);
                tail_put<true>(out, 3 * c + 2, B8);
            }
        }
    }
}
#endif

}  // namespace tmf
