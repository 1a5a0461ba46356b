// dgesdd-route second passes of embed and extract (tmfwm_fixup.h) for one block size, TMF_B:
// compiled once per size (tmfwm_fixup<b>.o), so that the sizes compile in parallel.
#include "tmfwm_fixup.h"

#ifndef TMF_B
#error "TMF_B: the block size of this translation unit"
#endif

namespace tmf {

template <int B>
__global__ __launch_bounds__(64) void embed_fixup_kernel(EmbedArgs a, const uint32_t *__restrict__ list, const uint32_t *__restrict__ count)
{
    fixup_walk<B, FixLds<B>>(list, count, [&](auto par, uint32_t id, FixLds<B> &f, int gl) {
        embed_fix_block<B, typename decltype(par)::Par, decltype(par)::G>(a, id, f, gl);
    });
}

// embed's key variant (a.key_out set): each listed block's S[0] into its key entry as well
template <int B>
__global__ __launch_bounds__(64) void embed_key_fixup_kernel(EmbedArgs a, const uint32_t *__restrict__ list,
                                                             const uint32_t *__restrict__ count)
{
    fixup_walk<B, FixLds<B>>(list, count, [&](auto par, uint32_t id, FixLds<B> &f, int gl) {
        embed_fix_block<B, typename decltype(par)::Par, decltype(par)::G, true>(a, id, f, gl);
    });
}

template <int B>
__global__ __launch_bounds__(64) void extract_fixup_kernel(ExtractArgs a, const uint32_t *__restrict__ list,
                                                           const uint32_t *__restrict__ count)
{
    fixup_walk<B, FixLdsS<B>>(list, count, [&](auto par, uint32_t id, FixLdsS<B> &f, int gl) {
        extract_fix_block<B, typename decltype(par)::Par, decltype(par)::G>(a, id, f, gl);
    });
}

template <int B>
hipError_t embed_fixup_b(const EmbedArgs &a, const uint32_t *list, const uint32_t *count, int64_t max_entries, hipStream_t st)
{
    return launch_fixup<B>(embed_fixup_kernel<B>, a, list, count, max_entries, st);
}

template <int B>
hipError_t embed_key_fixup_b(const EmbedArgs &a, const uint32_t *list, const uint32_t *count, int64_t max_entries, hipStream_t st)
{
    return launch_fixup<B>(embed_key_fixup_kernel<B>, a, list, count, max_entries, st);
}

template <int B>
hipError_t extract_fixup_b(const ExtractArgs &a, const uint32_t *list, const uint32_t *count, int64_t max_entries, hipStream_t st)
{
    return launch_fixup<B>(extract_fixup_kernel<B>, a, list, count, max_entries, st);
}

template hipError_t embed_fixup_b<TMF_B>(const EmbedArgs &, const uint32_t *, const uint32_t *, int64_t, hipStream_t);
template hipError_t embed_key_fixup_b<TMF_B>(const EmbedArgs &, const uint32_t *, const uint32_t *, int64_t, hipStream_t);
template hipError_t extract_fixup_b<TMF_B>(const ExtractArgs &, const uint32_t *, const uint32_t *, int64_t, hipStream_t);

}  // namespace tmf
