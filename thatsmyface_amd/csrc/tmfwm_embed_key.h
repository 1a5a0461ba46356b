// The extraction key out of the embed pass: which blocks' key entry the embed
// kernels may store themselves.
//
// Before the blend the byte certificate holds the top singular value of the original's DCT block
// as the interval [f32(max(sigma_1 - tE, 0)), f32(sigma_1 + tE)]: tE = 2^-45 sigma_1 (K = 256) for
// a certified block, 0 for a zero, flat or flagged one.  LAPACK's f64 sigma_1 lies inside it -- the
// assumption the hybrid route's bytes rest on -- and rounding to f32 is monotone, so when both
// ends are one float that float is np.linalg.svd's f32 S[0]: the key entry.  When they differ
// (a float midpoint lies within tE of sigma_1: about 2^-20 of the blocks) the block goes to the
// dgesdd route, whose pass stores its own S[0].
//
// Compiles for the host as well (tests/native/embed_key_host.cpp), like tmfwm_colour_tail.h.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define TMF_EK_FN __host__ __device__ __forceinline__
#else
#define TMF_EK_FN inline
#endif

namespace tmf {

// The embed kernels' key variant per block size: true stores the key from the strip pass (and
// b = 8's list pass) as above; false would compose the call of today's embed passes and today's
// map passes, as the rank-1 routes do.  Every size's key variant keeps its plain sibling's
// scratch and waves per SIMD (profiles/embed_key/resource_usage.txt), so every size is fused.
template <int B>
constexpr bool kEmbedKeyFused = true;

struct KeyDecision {
    bool decided;
    float key;
};

TMF_EK_FN uint32_t key_bits(float x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_uint(x);
#else
    uint32_t u;
    memcpy(&u, &x, sizeof u);
    return u;
#endif
}

// tl, th: the two pre-blend ends of the top triplet (both >= +0).  Decided iff they are the same
// finite float, compared bitwise.
TMF_EK_FN KeyDecision embed_key_decide(float tl, float th)
{
    const uint32_t l = key_bits(tl), h = key_bits(th);
    return {l == h && (l & 0x7F800000u) != 0x7F800000u, tl};
}

// the two ends as the kernels form them (tmfwm_blocks.h) from the f64 sigma_1 and tE
TMF_EK_FN KeyDecision embed_key_of(double sigma, double tE)
{
    const double lo = sigma - tE;
    return embed_key_decide((float)(lo > 0.0 ? lo : 0.0), (float)(sigma + tE));
}

}  // namespace tmf
