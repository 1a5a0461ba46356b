// Strip passes of the ragged calls (tmfwm_ragged.h) for one block size, TMF_B: the
// Makefile compiles this file once per size (tmfwm_ragged_strip<b>.o), b = 8 under the same
// max-ILP scheduler as its single-size sibling embed_kernel<8> (tmfwm_embed8.hip).  The keyed
// kernels' single-size siblings (tmfwm_keyed.hip) are compiled under the default scheduler, and
// max-ILP stretches keyed_sigma<8> to 168 VGPRs and scratch; so at b = 8 the Makefile makes two
// objects of this file: TMF_RAGGED_PART = 1, the embed / extract kernels under max-ILP, and
// TMF_RAGGED_PART = 2, the keyed kernels under the default scheduler (unset: both).
//
// With -DTMF_RAGGED_ALPHAS=1 the unit holds the per-frame form of these kernels instead
// (tmfwm_ragged.h: TMF_RAGGED_NAME, and the views read the frame's alpha from the alpha table --
// one more scalar load of the wave); the key maps take no alpha and have no such form.
//
// One workgroup (one wave) per strip on a flat 1-D grid.  The wave finds its frame in the
// table's wave prefix -- blockIdx.x is wave-uniform, so the search and what it yields are scalar
// loads and SGPRs -- and runs embed_blocks<B, false> / extract_sigmas<B, kPowerIters> /
// keyed_sigma<B, kPowerIters> on that frame's one-frame view.
#include "tmfwm_keyed.h"
#include "tmfwm_passes.h"
#include "tmfwm_ragged_strips.h"

#ifndef TMF_B
#error "TMF_B: the block size of this translation unit"
#endif
#ifndef TMF_RAGGED_PART
#define TMF_RAGGED_PART 3  // bit 0: the embed / extract kernels, bit 1: the keyed kernels
#endif

namespace tmf {

#if TMF_RAGGED_PART & 1
template <int B>
__global__ __launch_bounds__(64, kEmbedWaves<B>) void TMF_RAGGED_NAME(embed_ragged, _kernel)(RaggedArgs r)
{
    constexpr int BPW = Geo<B>::BPW, TS = kEmbedTS<B>;
    __shared__ __attribute__((aligned(16))) float lds_all[BPW * TS + kHiPad<B> + kLds2Floats<B>];  // as embed_kernel
    float *lds = lds_all, *lds2 = lds_all + BPW * TS + kHiPad<B>;
    RaggedFrameK *f = ragged_wave_frame(r);
    const EmbedArgs a = ragged_embed_view<kRaggedAlphas>(r, f);
    uint32_t id;
    const StripPos pos = ragged_strip_pos<B>(f, id);
    embed_blocks<B, false>(a, pos, id, lds, lds2);
}

// embed's key variant (tmfwm_embed_key.h): the frame's key pointer from the call's side table
// (r.keys, indexed as r.frames: the 64-byte table entry has no room for a second output)
template <int B>
__global__ __launch_bounds__(64, kEmbedWaves<B>) void TMF_RAGGED_NAME(embed_key_ragged, _kernel)(RaggedKeyArgs r)
{
    constexpr int BPW = Geo<B>::BPW, TS = kEmbedTS<B>;
    __shared__ __attribute__((aligned(16))) float lds_all[BPW * TS + kHiPad<B> + kLds2Floats<B>];  // as embed_kernel
    float *lds = lds_all, *lds2 = lds_all + BPW * TS + kHiPad<B>;
    RaggedFrameK *f = ragged_wave_frame(r);
    EmbedArgs a = ragged_embed_view<kRaggedAlphas>(r, f);
    a.key_out = ragged_key_const(r.keys)[f - ragged_const(r.frames)];
    uint32_t id;
    const StripPos pos = ragged_strip_pos<B>(f, id);
    embed_blocks<B, false, true>(a, pos, id, lds, lds2);
}

template <int B>
__global__ __launch_bounds__(64, (B > 8 ? 2 : kExtract8Waves)) void TMF_RAGGED_NAME(extract_ragged, _kernel)(RaggedArgs r)
{
    constexpr int L = Geo<B>::L, BPW = Geo<B>::BPW, LD = B + 1;
    __shared__ float lds[BPW * B * LD];
    const int lane = threadIdx.x & 63, g = lane / L, q = lane % L;
    RaggedFrameK *f = ragged_wave_frame(r);
    const ExtractArgs a = ragged_extract_view<kRaggedAlphas>(r, f);
    uint32_t id;
    const StripPos pos = ragged_strip_pos<B>(f, id);
    float sw, so;
    bool ok;
    extract_sigmas<B, kPowerIters>(a, pos, lds + g * B * LD, q, sw, so, ok);
    if (!pos.valid || q != 0) return;
    if (!ok) {  // the enclosure did not decide f32(sigma_1): the dgesdd route
        a.fb_list[atomicAdd(a.fb_count, 1u)] = id;
        return;
    }
    a.out[(int64_t)pos.bi * a.nbw + pos.bj] = extract_byte(sw, so, a.alpha32);
}

template <int B>
hipError_t TMF_RAGGED_NAME(embed_ragged, _b)(const RaggedArgs &r, unsigned waves, hipStream_t st)
{
    hipLaunchKernelGGL((TMF_RAGGED_NAME(embed_ragged, _kernel)<B>), dim3(waves), dim3(64), 0, st, r);
    return hipGetLastError();
}

template <int B>
hipError_t TMF_RAGGED_NAME(embed_key_ragged, _b)(const RaggedKeyArgs &r, unsigned waves, hipStream_t st)
{
    hipLaunchKernelGGL((TMF_RAGGED_NAME(embed_key_ragged, _kernel)<B>), dim3(waves), dim3(64), 0, st, r);
    return hipGetLastError();
}

template <int B>
hipError_t TMF_RAGGED_NAME(extract_ragged, _b)(const RaggedArgs &r, unsigned waves, hipStream_t st)
{
    hipLaunchKernelGGL((TMF_RAGGED_NAME(extract_ragged, _kernel)<B>), dim3(waves), dim3(64), 0, st, r);
    return hipGetLastError();
}

template hipError_t TMF_RAGGED_NAME(embed_ragged, _b)<TMF_B>(const RaggedArgs &, unsigned, hipStream_t);
template hipError_t TMF_RAGGED_NAME(embed_key_ragged, _b)<TMF_B>(const RaggedKeyArgs &, unsigned, hipStream_t);
template hipError_t TMF_RAGGED_NAME(extract_ragged, _b)<TMF_B>(const RaggedArgs &, unsigned, hipStream_t);
#endif

#if TMF_RAGGED_PART & 2
// keyed extraction (tmfwm_keyed.h): keyed_sigma on the frame's one image; an undecided block goes
// straight to the dgesdd route, a decided one through keyed_store on the one-frame view
template <int B, bool MAP, int PX, bool PF>
TMF_DEVI void keyed_ragged_strip(const RaggedArgs &r)
{
    constexpr int L = Geo<B>::L, BPW = Geo<B>::BPW, LD = B + 1;
    __shared__ float lds[BPW * B * LD];
    const int lane = threadIdx.x & 63, g = lane / L, q = lane % L;
    RaggedFrameK *f = ragged_wave_frame(r);
    const KeyedArgs a = ragged_keyed_view<PF>(r, f);
    uint32_t id;
    const StripPos pos = ragged_strip_pos<B>(f, id);
    float s;
    bool ok;
    keyed_sigma<B, kPowerIters, PX>(a, pos, lds + g * B * LD, q, s, ok);
    if (!pos.valid || q != 0) return;
    if (!ok) {
        a.fb_list[atomicAdd(a.fb_count, 1u)] = id;
        return;
    }
    keyed_store<MAP>(a, 0, pos.bi, pos.bj, s);
}

#if !TMF_RAGGED_ALPHAS
template <int B>
__global__ __launch_bounds__(64, kKeyedWaves<B>) void sigma1_map_ragged_kernel(RaggedArgs r)
{
    keyed_ragged_strip<B, true, 3, kRaggedAlphas>(r);
}
#endif

template <int B>
__global__ __launch_bounds__(64, kKeyedWaves<B>) void TMF_RAGGED_NAME(extract_keyed_ragged, _kernel)(RaggedArgs r)
{
    keyed_ragged_strip<B, false, 3, kRaggedAlphas>(r);
}

// frames of 4-byte pixels (R G B pad), read in place: kernels of their own beside the 3-byte ones
#if !TMF_RAGGED_ALPHAS
template <int B>
__global__ __launch_bounds__(64, kKeyedWaves<B>) void sigma1_map_ragged_px4_kernel(RaggedArgs r)
{
    keyed_ragged_strip<B, true, 4, kRaggedAlphas>(r);
}
#endif

template <int B>
__global__ __launch_bounds__(64, kKeyedWaves<B>) void TMF_RAGGED_NAME(extract_keyed_ragged, _px4_kernel)(RaggedArgs r)
{
    keyed_ragged_strip<B, false, 4, kRaggedAlphas>(r);
}

#if !TMF_RAGGED_ALPHAS
template <int B>
hipError_t sigma1_map_ragged_b(const RaggedArgs &r, unsigned waves, hipStream_t st, int px)
{
    hipLaunchKernelGGL((px == 4 ? sigma1_map_ragged_px4_kernel<B> : sigma1_map_ragged_kernel<B>), dim3(waves), dim3(64), 0, st, r);
    return hipGetLastError();
}

template hipError_t sigma1_map_ragged_b<TMF_B>(const RaggedArgs &, unsigned, hipStream_t, int);
#endif

template <int B>
hipError_t TMF_RAGGED_NAME(extract_keyed_ragged, _b)(const RaggedArgs &r, unsigned waves, hipStream_t st, int px)
{
    hipLaunchKernelGGL((px == 4 ? TMF_RAGGED_NAME(extract_keyed_ragged, _px4_kernel)<B> : TMF_RAGGED_NAME(extract_keyed_ragged, _kernel)<B>),
                       dim3(waves), dim3(64), 0, st, r);
    return hipGetLastError();
}

template hipError_t TMF_RAGGED_NAME(extract_keyed_ragged, _b)<TMF_B>(const RaggedArgs &, unsigned, hipStream_t, int);
#endif

}  // namespace tmf
