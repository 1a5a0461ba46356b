// TEST-ONLY: the f32 colour-tail decision (thatsmyface_amd/csrc/tmfwm_colour_tail.h) compiled for
// the host CPU and swept against the exact tail, so that tests/test_colour_tail.py can check its
// soundness over all 2^24 colours without a GPU.  Built by that test; never shipped.
// With -DCT_MAIN: a stand-alone program running a strided sweep (for a host sanitiser build).
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../thatsmyface_amd/csrc/tmfwm_colour_tail.h"

namespace {

// ---- the exact tail, restated from tmfwm_device.h (unit_from_u8, luma, chroma, colour_inv);
// built with -ffp-contract=off, fused operations only where written
constexpr float kUnitHi = 0.003921568859368562698f, kUnitLo = -2.3191758e-10f;
inline float unit_from_u8(uint32_t v)
{
    const float x = (float)v;
    return fmaf(x, kUnitHi, x * kUnitLo);
}
inline float luma(uint32_t R, uint32_t G, uint32_t B)
{
    const double r = unit_from_u8(R), g = unit_from_u8(G), b = unit_from_u8(B);
    return (float)fma(0.114, b, fma(0.299, r, 0.587 * g));
}
inline void chroma(uint32_t R, uint32_t G, uint32_t B, float &cbs, float &crs)
{
    const double r = unit_from_u8(R), g = unit_from_u8(G), b = unit_from_u8(B);
    cbs = (float)fma(0.5, b, fma(-0.169, r, -0.331 * g)) + 0.5f;
    crs = (float)fma(-0.081, b, fma(0.5, r, -0.419 * g)) + 0.5f;
}
inline uint32_t u8_from_unit(float f)
{
    f = f > 0.0f ? f : 0.0f;  // v_med3_f32(f, 0, 1) up to the sign of a zero
    f = f < 1.0f ? f : 1.0f;
    return (uint32_t)(f * 255.0f);
}
inline void colour_inv(float y, float cbs, float crs, uint32_t &R, uint32_t &G, uint32_t &B)
{
    const double Y = y, CB = cbs - 0.5f, CR = crs - 0.5f;
    R = u8_from_unit((float)fma(1.403, CR, Y));
    G = u8_from_unit((float)fma(-0.714, CR, Y + -0.344 * CB));
    B = u8_from_unit((float)(Y + 1.773 * CB));
}

struct Stats {
    long long evals = 0, accepted = 0, bad = 0;
    uint32_t bad_colour = 0, bad_yl = 0, bad_dy = 0;
};

// one lower end with the four widths {0, one ulp, 2^-20, 2^-12}
inline void check_yl(uint32_t R0, uint32_t G0, uint32_t B0, float cbs, float crs, float yl, Stats &s)
{
    uint32_t Re, Ge, Be;
    colour_inv(yl, cbs, crs, Re, Ge, Be);
    const float yhs[4] = {yl, nextafterf(yl, INFINITY), yl + 0x1p-20f, yl + 0x1p-12f};
    for (int k = 0; k < 4; ++k) {
        const float yh = yhs[k], dy = yh - yl;
        uint32_t R, G, B;
        ++s.evals;
        if (!tmf::colour_tail_fast(R0, G0, B0, yl, dy, R, G, B)) continue;
        ++s.accepted;
        uint32_t Rh, Gh, Bh;
        colour_inv(yh, cbs, crs, Rh, Gh, Bh);
        if (R != Re || G != Ge || B != Be || R != Rh || G != Gh || B != Bh) {
            if (s.bad++ == 0) {
                s.bad_colour = R0 | G0 << 8 | B0 << 16;
                memcpy(&s.bad_yl, &yl, 4);
                memcpy(&s.bad_dy, &dy, 4);
            }
        }
    }
}

void sweep_colour(uint32_t col, const float *offs, int noffs, const float *absy, int nabs, const float *solve, int nsolve, Stats &s)
{
    const uint32_t R0 = col & 255u, G0 = (col >> 8) & 255u, B0 = col >> 16;
    float cbs, crs;
    chroma(R0, G0, B0, cbs, crs);
    const float y0 = luma(R0, G0, B0);
    for (int i = 0; i < noffs; ++i) check_yl(R0, G0, B0, cbs, crs, y0 + offs[i], s);  // luma and luma +- levels
    for (int i = 0; i < nabs; ++i) check_yl(R0, G0, B0, cbs, crs, absy[i], s);        // clipping, the alpha edges
    // lower ends solved to put each channel's scaled value at m + e kDelta, m the two byte
    // boundaries around the channel's own value, e = solve[]
    const double CB = cbs - 0.5f, CR = crs - 0.5f;
    const double w[3] = {1.403 * CR, -0.714 * CR + -0.344 * CB, 1.773 * CB};
    for (int ch = 0; ch < 3; ++ch) {
        const double q0 = 255.0 * ((double)y0 + w[ch]);
        const double nb = floor(q0 < 0.0 ? 0.0 : q0 > 255.0 ? 255.0 : q0);
        for (int m = 0; m < 2; ++m)
            for (int i = 0; i < nsolve; ++i) {
                const double target = nb + m + (double)solve[i] * (double)tmf::ct::kDelta;
                check_yl(R0, G0, B0, cbs, crs, (float)((double)y0 + (target - q0) / 255.0), s);
            }
    }
}

}  // namespace

extern "C" {

// colours c0, c0 + step, ... < c1; out = {evals, accepted, bad, first bad colour, its yl bits, its dy bits}
void ct_sweep(uint32_t c0, uint32_t c1, uint32_t step, const float *offs, int noffs, const float *absy, int nabs,
              const float *solve, int nsolve, long long *out)
{
    long long evals = 0, accepted = 0, bad = 0;
    long long first[3] = {-1, 0, 0};
#pragma omp parallel for schedule(static) reduction(+ : evals, accepted, bad)
    for (long long c = c0; c < (long long)c1; c += step) {
        Stats s;
        sweep_colour((uint32_t)c, offs, noffs, absy, nabs, solve, nsolve, s);
        evals += s.evals;
        accepted += s.accepted;
        bad += s.bad;
        if (s.bad) {
#pragma omp critical
            if (first[0] < 0) first[0] = s.bad_colour, first[1] = s.bad_yl, first[2] = s.bad_dy;
        }
    }
    out[0] = evals, out[1] = accepted, out[2] = bad, out[3] = first[0], out[4] = first[1], out[5] = first[2];
}

// every colour once with yl = its luma + u * spread, u in [-1, 1) from a hash of the colour:
// out = {pixels, accepted, bad}
void ct_accept_rate(float spread, float dy, long long *out)
{
    long long accepted = 0, bad = 0;
#pragma omp parallel for schedule(static) reduction(+ : accepted, bad)
    for (long long c = 0; c < (1ll << 24); ++c) {
        const uint32_t R0 = c & 255u, G0 = (c >> 8) & 255u, B0 = (uint32_t)(c >> 16);
        uint32_t h = (uint32_t)c * 2654435761u;
        h ^= h >> 15, h *= 2246822519u, h ^= h >> 13;
        const float u = (float)(h >> 8) * 0x1p-23f - 1.0f;
        const float yl = luma(R0, G0, B0) + u * spread, yh = yl + dy;
        uint32_t R, G, B;
        if (!tmf::colour_tail_fast(R0, G0, B0, yl, yh - yl, R, G, B)) continue;
        ++accepted;
        float cbs, crs;
        chroma(R0, G0, B0, cbs, crs);
        uint32_t Re, Ge, Be, Rh, Gh, Bh;
        colour_inv(yl, cbs, crs, Re, Ge, Be);
        colour_inv(yh, cbs, crs, Rh, Gh, Bh);
        bad += R != Re || G != Ge || B != Be || R != Rh || G != Gh || B != Bh;
    }
    out[0] = 1ll << 24, out[1] = accepted, out[2] = bad;
}

// one evaluation: returns accept, bytes in rgb[3]
int ct_fast(uint32_t R0, uint32_t G0, uint32_t B0, float yl, float dy, uint32_t *rgb)
{
    return tmf::colour_tail_fast(R0, G0, B0, yl, dy, rgb[0], rgb[1], rgb[2]) ? 1 : 0;
}

float ct_delta(void) { return tmf::ct::kDelta; }
}

#ifdef CT_MAIN
int main()
{
    const float offs[] = {0.0f, 0.7f / 255, -1.3f / 255, 4.6f / 255, -9.1f / 255};
    const float absy[] = {-8.0f, -1.0f, -1e-4f, 1.0f + 1e-4f, 2.0f, 8.0f};
    const float solve[] = {-2.0f, -1.0f, -0.25f, 0.25f, 1.0f, 2.0f};
    long long out[6];
    ct_sweep(0, 1u << 24, 257, offs, 5, absy, 6, solve, 6, out);
    printf("{\"evals\": %lld, \"accepted\": %lld, \"bad\": %lld}\n", out[0], out[1], out[2]);
    return out[2] != 0;
}
#endif
