// dgesdd-route second passes of the ragged calls (tmfwm_ragged.h) for one block size,
// TMF_RAGGED_B: compiled once per size (tmfwm_ragged_fixup<b>.o), as their single-size siblings
// are (tmfwm_fixup<b>.hip).  The grid policy is embed_fixup_kernel's: a wave per block for a
// short list, groups of G lanes for a long one; each listed id's frame is found in the table's
// block prefix and embed_fix_block / extract_fix_block run on that frame's one-frame view.
#include "tmfwm_fixup.h"
#include "tmfwm_ragged.h"

#ifndef TMF_RAGGED_B
#error "TMF_RAGGED_B: the block size of this translation unit"
#endif

namespace tmf {

// the frame of chunk-relative block id `id`
TMF_DEVI const RaggedFrame *ragged_block_frame(const RaggedArgs &r, uint32_t id)
{
    return r.frames + ragged_find(r.nframes, id, [&](int i) { return r.frames[i].block0; });
}

template <int B, class Par, int G>
TMF_DEVI void embed_ragged_fix(const RaggedArgs &r, uint32_t id, FixLds<B> &f, int gl)
{
    const RaggedFrame *fr = ragged_block_frame(r, id);
    const EmbedArgs a = ragged_embed_view(r, fr);
    embed_fix_block<B, Par, G>(a, id - fr->block0, f, gl);
}

template <int B, class Par, int G>
TMF_DEVI void extract_ragged_fix(const RaggedArgs &r, uint32_t id, FixLdsS<B> &f, int gl)
{
    const RaggedFrame *fr = ragged_block_frame(r, id);
    const ExtractArgs a = ragged_extract_view(r, fr);
    extract_fix_block<B, Par, G>(a, id - fr->block0, f, gl);
}

template <int B>
__global__ __launch_bounds__(64) void embed_ragged_fixup_kernel(RaggedArgs r, const uint32_t *__restrict__ list,
                                                                const uint32_t *__restrict__ count)
{
    constexpr int G = kFixLanes<B>, NG = 64 / G;
    __shared__ FixLds<B> fl[NG];
    const uint32_t n = *count;
    if (n <= gridDim.x) {
        if (blockIdx.x < n) embed_ragged_fix<B, lp::WavePar, 64>(r, list[blockIdx.x], fl[0], (int)threadIdx.x);
        return;
    }
    const int gl = lp::GroupPar<G>::lane(), grp = (int)(threadIdx.x / G);
    for (uint32_t t0 = blockIdx.x * NG; t0 < n; t0 += gridDim.x * NG) {
        const uint32_t t = t0 + (uint32_t)grp;
        if (t < n) embed_ragged_fix<B, lp::GroupPar<G>, G>(r, list[t], fl[grp], gl);
    }
}

template <int B>
__global__ __launch_bounds__(64) void extract_ragged_fixup_kernel(RaggedArgs r, const uint32_t *__restrict__ list,
                                                                  const uint32_t *__restrict__ count)
{
    constexpr int G = kFixLanes<B>, NG = 64 / G;
    __shared__ FixLdsS<B> fl[NG];
    const uint32_t n = *count;
    if (n <= gridDim.x) {
        if (blockIdx.x < n) extract_ragged_fix<B, lp::WavePar, 64>(r, list[blockIdx.x], fl[0], (int)threadIdx.x);
        return;
    }
    const int gl = lp::GroupPar<G>::lane(), grp = (int)(threadIdx.x / G);
    for (uint32_t t0 = blockIdx.x * NG; t0 < n; t0 += gridDim.x * NG) {
        const uint32_t t = t0 + (uint32_t)grp;
        if (t < n) extract_ragged_fix<B, lp::GroupPar<G>, G>(r, list[t], fl[grp], gl);
    }
}

#define TMF_CAT_(a, b) a##b
#define TMF_CAT(a, b) TMF_CAT_(a, b)

hipError_t TMF_CAT(launch_embed_ragged_fixup_, TMF_RAGGED_B)(const RaggedArgs &r, const uint32_t *list, const uint32_t *count,
                                                             int64_t max_entries, hipStream_t st)
{
    hipLaunchKernelGGL((embed_ragged_fixup_kernel<TMF_RAGGED_B>), dim3(fixup_grid<TMF_RAGGED_B>(max_entries)), dim3(64), 0, st, r, list,
                       count);
    return hipGetLastError();
}

hipError_t TMF_CAT(launch_extract_ragged_fixup_, TMF_RAGGED_B)(const RaggedArgs &r, const uint32_t *list, const uint32_t *count,
                                                               int64_t max_entries, hipStream_t st)
{
    hipLaunchKernelGGL((extract_ragged_fixup_kernel<TMF_RAGGED_B>), dim3(fixup_grid<TMF_RAGGED_B>(max_entries)), dim3(64), 0, st, r,
                       list, count);
    return hipGetLastError();
}

}  // namespace tmf
