// Keyed extraction: device functions shared by the strip / list passes
// (tmfwm_keyed.hip) and the dgesdd-route passes (tmfwm_keyed_fixup.hip).
//
// extract's byte depends on the original image only through f32(sigma_1) of each of its blocks.
// sigma1_map stores that float per block -- the key -- and extract_keyed takes the key in place
// of the original's pixels.  Both run the pair path's arithmetic on one image: the certified
// enclosure (sigma1_certified) where it decides, the dgesdd route where it does not, so a key
// entry is np.linalg.svd's f32 S[0] on every route.
#pragma once
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

}  // namespace tmf
