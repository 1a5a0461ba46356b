// dgesdd-route second passes of the ragged calls (tmfwm_ragged.h) for one block size,
// TMF_B: compiled once per size (tmfwm_ragged_fixup<b>.o), as their single-size siblings are
// (tmfwm_fixup.hip).  The walk over the list is theirs (fixup_walk); each listed id's frame is found
// in the table's block prefix and embed_fix_block / extract_fix_block / keyed_fix_block run on
// that frame's one-frame view.
//
// With -DTMF_RAGGED_ALPHAS=1 the unit holds the per-frame form of these kernels instead
// (tmfwm_ragged.h): the alpha is the listed block's frame's, per lane, since a fixup wave holds
// blocks of several frames.
#include "tmfwm_fixup.h"
#include "tmfwm_keyed.h"
#include "tmfwm_ragged.h"

#ifndef TMF_B
#error "TMF_B: the block size of this translation unit"
#endif

namespace tmf {

// the frame of chunk-relative block id `id`
TMF_DEVI const RaggedFrame *ragged_block_frame(const RaggedArgs &r, uint32_t id)
{
    return r.frames + ragged_find(r.nframes, id, [&](int i) { return r.frames[i].block0; });
}

template <int B, class Par, int G, bool PF>
TMF_DEVI void embed_ragged_fix(const RaggedArgs &r, uint32_t id, FixLds<B> &f, int gl)
{
    const RaggedFrame *fr = ragged_block_frame(r, id);
    const EmbedArgs a = ragged_embed_view<PF>(r, fr);
    embed_fix_block<B, Par, G>(a, id - fr->block0, f, gl);
}

// embed's key variant: the frame's key pointer from the call's side table
template <int B, class Par, int G, bool PF>
TMF_DEVI void embed_key_ragged_fix(const RaggedKeyArgs &r, uint32_t id, FixLds<B> &f, int gl)
{
    const RaggedFrame *fr = ragged_block_frame(r, id);
    EmbedArgs a = ragged_embed_view<PF>(r, fr);
    a.key_out = r.keys[fr - r.frames];
    embed_fix_block<B, Par, G, true>(a, id - fr->block0, f, gl);
}

template <int B, class Par, int G, bool PF>
TMF_DEVI void extract_ragged_fix(const RaggedArgs &r, uint32_t id, FixLdsS<B> &f, int gl)
{
    const RaggedFrame *fr = ragged_block_frame(r, id);
    const ExtractArgs a = ragged_extract_view<PF>(r, fr);
    extract_fix_block<B, Par, G>(a, id - fr->block0, f, gl);
}

template <int B>
__global__ __launch_bounds__(64) void TMF_RAGGED_NAME(embed_ragged, _fixup_kernel)(RaggedArgs r, const uint32_t *__restrict__ list,
                                                                const uint32_t *__restrict__ count)
{
    fixup_walk<B, FixLds<B>>(list, count, [&](auto par, uint32_t id, FixLds<B> &f, int gl) {
        embed_ragged_fix<B, typename decltype(par)::Par, decltype(par)::G, kRaggedAlphas>(r, id, f, gl);
    });
}

template <int B>
__global__ __launch_bounds__(64) void TMF_RAGGED_NAME(embed_key_ragged, _fixup_kernel)(RaggedKeyArgs r, const uint32_t *__restrict__ list,
                                                                    const uint32_t *__restrict__ count)
{
    fixup_walk<B, FixLds<B>>(list, count, [&](auto par, uint32_t id, FixLds<B> &f, int gl) {
        embed_key_ragged_fix<B, typename decltype(par)::Par, decltype(par)::G, kRaggedAlphas>(r, id, f, gl);
    });
}

template <int B>
__global__ __launch_bounds__(64) void TMF_RAGGED_NAME(extract_ragged, _fixup_kernel)(RaggedArgs r, const uint32_t *__restrict__ list,
                                                                  const uint32_t *__restrict__ count)
{
    fixup_walk<B, FixLdsS<B>>(list, count, [&](auto par, uint32_t id, FixLdsS<B> &f, int gl) {
        extract_ragged_fix<B, typename decltype(par)::Par, decltype(par)::G, kRaggedAlphas>(r, id, f, gl);
    });
}

// keyed extraction (tmfwm_keyed.h): keyed_fix_block on the frame's one image
template <int B, bool MAP, int PX, bool PF>
TMF_DEVI void keyed_ragged_fixup(const RaggedArgs &r, const uint32_t *__restrict__ list, const uint32_t *__restrict__ count)
{
    fixup_walk<B, FixLdsS<B>>(list, count, [&](auto par, uint32_t id, FixLdsS<B> &f, int gl) {
        const RaggedFrame *fr = ragged_block_frame(r, id);
        const KeyedArgs a = ragged_keyed_view<PF>(r, fr);
        keyed_fix_block<B, typename decltype(par)::Par, decltype(par)::G, MAP, PX>(a, id - fr->block0, f, gl);
    });
}

#if !TMF_RAGGED_ALPHAS
template <int B>
__global__ __launch_bounds__(64) void sigma1_ragged_fixup_kernel(RaggedArgs r, const uint32_t *__restrict__ list,
                                                                 const uint32_t *__restrict__ count)
{
    keyed_ragged_fixup<B, true, 3, kRaggedAlphas>(r, list, count);
}
#endif

// the waves per SIMD of extract_keyed_fixup_kernel<B>: the frame's key and tile pointers are per
// lane here, which at b = 4 costs the two VGPRs that would otherwise drop it to 3
template <int B>
constexpr int kKeyedFixWaves = B <= 12 ? 4 : 3;

template <int B>
__global__ __launch_bounds__(64, kKeyedFixWaves<B>) void TMF_RAGGED_NAME(extract_keyed_ragged, _fixup_kernel)(RaggedArgs r, const uint32_t *__restrict__ list,
                                                                        const uint32_t *__restrict__ count)
{
    keyed_ragged_fixup<B, false, 3, kRaggedAlphas>(r, list, count);
}

// frames of 4-byte pixels (tmfwm_ragged_strip.hip): kernels of their own beside the 3-byte ones
#if !TMF_RAGGED_ALPHAS
template <int B>
__global__ __launch_bounds__(64) void sigma1_ragged_fixup_px4_kernel(RaggedArgs r, const uint32_t *__restrict__ list,
                                                                     const uint32_t *__restrict__ count)
{
    keyed_ragged_fixup<B, true, 4, kRaggedAlphas>(r, list, count);
}
#endif

template <int B>
__global__ __launch_bounds__(64, kKeyedFixWaves<B>) void TMF_RAGGED_NAME(extract_keyed_ragged, _fixup_px4_kernel)(RaggedArgs r, const uint32_t *__restrict__ list,
                                                                            const uint32_t *__restrict__ count)
{
    keyed_ragged_fixup<B, false, 4, kRaggedAlphas>(r, list, count);
}

#if !TMF_RAGGED_ALPHAS
template <int B>
hipError_t sigma1_ragged_fixup_b(const RaggedArgs &r, const uint32_t *list, const uint32_t *count, int64_t max_entries, hipStream_t st,
                                 int px)
{
    return launch_fixup<B>(px == 4 ? sigma1_ragged_fixup_px4_kernel<B> : sigma1_ragged_fixup_kernel<B>, r, list, count, max_entries, st);
}

template hipError_t sigma1_ragged_fixup_b<TMF_B>(const RaggedArgs &, const uint32_t *, const uint32_t *, int64_t, hipStream_t, int);
#endif

template <int B>
hipError_t TMF_RAGGED_NAME(extract_keyed_ragged, _fixup_b)(const RaggedArgs &r, const uint32_t *list, const uint32_t *count, int64_t max_entries,
                                        hipStream_t st, int px)
{
    return launch_fixup<B>(px == 4 ? TMF_RAGGED_NAME(extract_keyed_ragged, _fixup_px4_kernel)<B> : TMF_RAGGED_NAME(extract_keyed_ragged, _fixup_kernel)<B>, r, list, count,
                           max_entries, st);
}

template <int B>
hipError_t TMF_RAGGED_NAME(embed_ragged, _fixup_b)(const RaggedArgs &r, const uint32_t *list, const uint32_t *count, int64_t max_entries, hipStream_t st)
{
    return launch_fixup<B>(TMF_RAGGED_NAME(embed_ragged, _fixup_kernel)<B>, r, list, count, max_entries, st);
}

template <int B>
hipError_t TMF_RAGGED_NAME(embed_key_ragged, _fixup_b)(const RaggedKeyArgs &r, const uint32_t *list, const uint32_t *count, int64_t max_entries, hipStream_t st)
{
    return launch_fixup<B>(TMF_RAGGED_NAME(embed_key_ragged, _fixup_kernel)<B>, r, list, count, max_entries, st);
}

template <int B>
hipError_t TMF_RAGGED_NAME(extract_ragged, _fixup_b)(const RaggedArgs &r, const uint32_t *list, const uint32_t *count, int64_t max_entries, hipStream_t st)
{
    return launch_fixup<B>(TMF_RAGGED_NAME(extract_ragged, _fixup_kernel)<B>, r, list, count, max_entries, st);
}

template hipError_t TMF_RAGGED_NAME(embed_ragged, _fixup_b)<TMF_B>(const RaggedArgs &, const uint32_t *, const uint32_t *, int64_t, hipStream_t);
template hipError_t TMF_RAGGED_NAME(embed_key_ragged, _fixup_b)<TMF_B>(const RaggedKeyArgs &, const uint32_t *, const uint32_t *, int64_t, hipStream_t);
template hipError_t TMF_RAGGED_NAME(extract_ragged, _fixup_b)<TMF_B>(const RaggedArgs &, const uint32_t *, const uint32_t *, int64_t, hipStream_t);
template hipError_t TMF_RAGGED_NAME(extract_keyed_ragged, _fixup_b)<TMF_B>(const RaggedArgs &, const uint32_t *, const uint32_t *, int64_t, hipStream_t, int);

}  // namespace tmf
