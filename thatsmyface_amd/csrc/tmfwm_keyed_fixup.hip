// dgesdd-route passes of keyed extraction (tmfwm_keyed.h) for one block size, TMF_KEYED_B:
// compiled once per size (tmfwm_keyed_fixup<b>.o), as tmfwm_ragged_fixup.hip is.  Each listed
// block's S[0] on the dgesdd route (np.linalg.svd's arithmetic), stored as its key entry
// (sigma1_fixup_kernel) or turned into its byte against the stored entry
// (extract_keyed_fixup_kernel).  The grid policy is extract_fixup_kernel's: a wave per block for
// a short list, groups of kFixLanes<B> lanes for a long one.
#include "tmfwm_fixup.h"
#include "tmfwm_keyed.h"

#ifndef TMF_KEYED_B
#error "TMF_KEYED_B: the block size of this translation unit"
#endif

namespace tmf {

template <int B, class Par, int G, bool MAP>
TMF_DEVI void keyed_fix_block(const KeyedArgs &a, uint32_t id, FixLdsS<B> &f, int gl)
{
    const uint32_t per_frame = (uint32_t)a.nbh * (uint32_t)a.nbw;
    int64_t fr;
    int bi, bj;
    block_of(id, per_frame, a.nbw, fr, bi, bj);
    fix_load_dct<B, G>(a.src + fr * a.frame_stride, a.W, bi, bj, f.D, gl);
    const int info = lp::svd_f32_ws<false, Par>(f.D, runtime_n(B), nullptr, f.S, nullptr, f.ws);  // :279-282
    if (info && gl == 0 && a.fb_bad) atomicAdd(a.fb_bad, 1u);
    const float s = f.S[0];
    group_sync();  // the LDS slots are reused by the next listed block
    if (gl == 0) keyed_store<MAP>(a, fr, bi, bj, s);
}

template <int B, bool MAP>
TMF_DEVI void keyed_fixup(const KeyedArgs &a, const uint32_t *__restrict__ list, const uint32_t *__restrict__ count)
{
    constexpr int G = kFixLanes<B>, NG = 64 / G;
    static_assert(G >= B, "a group holds one element of dbdsqr's vectors per lane");
    __shared__ FixLdsS<B> fl[NG];
    const uint32_t n = *count;
    if (n <= gridDim.x) {
        if (blockIdx.x < n) keyed_fix_block<B, lp::WavePar, 64, MAP>(a, list[blockIdx.x], fl[0], (int)threadIdx.x);
        return;
    }
    const int gl = lp::GroupPar<G>::lane(), grp = (int)(threadIdx.x / G);
    for (uint32_t t0 = blockIdx.x * NG; t0 < n; t0 += gridDim.x * NG) {
        const uint32_t t = t0 + (uint32_t)grp;
        if (t < n) keyed_fix_block<B, lp::GroupPar<G>, G, MAP>(a, list[t], fl[grp], gl);
    }
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

#define TMF_CAT_(a, b) a##b
#define TMF_CAT(a, b) TMF_CAT_(a, b)

hipError_t TMF_CAT(launch_sigma1_fixup_, TMF_KEYED_B)(const KeyedArgs &a, const uint32_t *list, const uint32_t *count,
                                                      int64_t max_entries, hipStream_t st)
{
    hipLaunchKernelGGL((sigma1_fixup_kernel<TMF_KEYED_B>), dim3(fixup_grid<TMF_KEYED_B>(max_entries)), dim3(64), 0, st, a, list, count);
    return hipGetLastError();
}

hipError_t TMF_CAT(launch_extract_keyed_fixup_, TMF_KEYED_B)(const KeyedArgs &a, const uint32_t *list, const uint32_t *count,
                                                             int64_t max_entries, hipStream_t st)
{
    hipLaunchKernelGGL((extract_keyed_fixup_kernel<TMF_KEYED_B>), dim3(fixup_grid<TMF_KEYED_B>(max_entries)), dim3(64), 0, st, a, list,
                       count);
    return hipGetLastError();
}

}  // namespace tmf
