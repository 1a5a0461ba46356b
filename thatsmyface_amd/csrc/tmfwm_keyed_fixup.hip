// dgesdd-route passes of keyed extraction (tmfwm_keyed.h) for one block size, TMF_B:
// compiled once per size (tmfwm_keyed_fixup<b>.o), as tmfwm_fixup.hip is.  Each listed
// block's S[0] on the dgesdd route (np.linalg.svd's arithmetic), stored as its key entry
// (sigma1_fixup_kernel) or turned into its byte against the stored entry
// (extract_keyed_fixup_kernel), on extract_fixup_kernel's walk over the list (fixup_walk).
#include "tmfwm_fixup.h"
#include "tmfwm_keyed.h"

#ifndef TMF_B
#error "TMF_B: the block size of this translation unit"
#endif

namespace tmf {

template <int B, bool MAP, int PX = 3>
TMF_DEVI void keyed_fixup(const KeyedArgs &a, const uint32_t *__restrict__ list, const uint32_t *__restrict__ count)
{
    fixup_walk<B, FixLdsS<B>>(list, count, [&](auto par, uint32_t id, FixLdsS<B> &f, int gl) {
        keyed_fix_block<B, typename decltype(par)::Par, decltype(par)::G, MAP, PX>(a, id, f, gl);
    });
}

template <int B>
__global__ __launch_bounds__(64) void sigma1_fixup_kernel(KeyedArgs a, const uint32_t *__restrict__ list,
                                                          const uint32_t *__restrict__ count)
{
    keyed_fixup<B, true>(a, list, count);
}

template <int B>
__global__ __launch_bounds__(64) void extract_keyed_fixup_kernel(KeyedArgs a, const uint32_t *__restrict__ list,
                                                                 const uint32_t *__restrict__ count)
{
    keyed_fixup<B, false>(a, list, count);
}

// frames of 4-byte pixels (tmfwm_keyed.hip): kernels of their own beside the 3-byte ones
template <int B>
__global__ __launch_bounds__(64) void sigma1_fixup_px4_kernel(KeyedArgs a, const uint32_t *__restrict__ list,
                                                              const uint32_t *__restrict__ count)
{
    keyed_fixup<B, true, 4>(a, list, count);
}

template <int B>
__global__ __launch_bounds__(64) void extract_keyed_fixup_px4_kernel(KeyedArgs a, const uint32_t *__restrict__ list,
                                                                     const uint32_t *__restrict__ count)
{
    keyed_fixup<B, false, 4>(a, list, count);
}

template <int B>
hipError_t sigma1_fixup_b(const KeyedArgs &a, const uint32_t *list, const uint32_t *count, int64_t max_entries, hipStream_t st, int px)
{
    return launch_fixup<B>(px == 4 ? sigma1_fixup_px4_kernel<B> : sigma1_fixup_kernel<B>, a, list, count, max_entries, st);
}

template <int B>
hipError_t extract_keyed_fixup_b(const KeyedArgs &a, const uint32_t *list, const uint32_t *count, int64_t max_entries, hipStream_t st,
                                 int px)
{
    return launch_fixup<B>(px == 4 ? extract_keyed_fixup_px4_kernel<B> : extract_keyed_fixup_kernel<B>, a, list, count, max_entries, st);
}

template hipError_t sigma1_fixup_b<TMF_B>(const KeyedArgs &, const uint32_t *, const uint32_t *, int64_t, hipStream_t, int);
template hipError_t extract_keyed_fixup_b<TMF_B>(const KeyedArgs &, const uint32_t *, const uint32_t *, int64_t, hipStream_t, int);

}  // namespace tmf
