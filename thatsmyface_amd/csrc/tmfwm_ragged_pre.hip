// The rank-1 routes of the ragged embed (tmfwm_embed_ragged_rank1; tmfwm_ragged.h)
// for one block size, TMF_B: the Makefile compiles this file once per size (tmfwm_ragged_pre<b>.o).
// Two kernels, each built as its single-size sibling is: the pre-pass (embed_rank1_kernel<b>,
// tmfwm_rank1.hip: the default scheduler) and the list pass of TMFWM_ROUTE_RANK1
// (embed_kernel<b, true>: at b = 8 under max-ILP, tmfwm_embed8.hip); so at b = 8 the Makefile
// makes two objects of this file, TMF_RAGGED_PRE_PART = 1 and 2 (unset: both).
//
// With -DTMF_RAGGED_ALPHAS=1 the unit holds the per-frame form of both kernels instead
// (tmfwm_ragged.h): the wave's frame's alpha from the alpha table, one more scalar load.
#include "tmfwm_rank1.h"
#include "tmfwm_ragged_strips.h"

#ifndef TMF_B
#error "TMF_B: the block size of this translation unit"
#endif
#ifndef TMF_RAGGED_PRE_PART
#define TMF_RAGGED_PRE_PART 3  // bit 0: the pre-pass, bit 1: the list pass
#endif

namespace tmf {

#if TMF_RAGGED_PRE_PART & 1
// One wave per strip on the flat grid, as embed_ragged_kernel: the pre-pass (tmfwm_rank1_body.h)
// on the frame's one-frame view.  A block it leaves goes to the frame's shard of its row
// (TMFWM_ROUTE_RANK1) or to the dgesdd-route list (TMFWM_ROUTE_RANK1_REFERENCE), by its
// chunk-relative id either way.
template <int B>
__global__ __launch_bounds__(64, kRank1Waves<B>) void TMF_RAGGED_NAME(embed_rank1_ragged, _kernel)(RaggedRank1Args rag)
{
    constexpr int L = Geo<B>::L, R = Geo<B>::R, LD = B + 1, NW = Geo<B>::NW;
    constexpr double u53 = 1.1102230246251565e-16;  // 2^-53
    constexpr float u24 = 5.9604644775390625e-08f;  // 2^-24
    __shared__ float lds[kRank1LdsFloats<B>];
    __shared__ uint32_t pix[kRank1PixWords<B>][64];
    const int lane = threadIdx.x & 63, g = lane / L, q = lane % L;
    float *tile = lds + g * B * LD;
    RaggedFrameK *f = ragged_wave_frame(rag);
    const EmbedArgs a = ragged_embed_view<kRaggedAlphas>(rag, f);
    uint32_t id;
    const StripPos pos = ragged_strip_pos<B>(f, id);
#define TMF_RANK1_LEFT                                                                                         \
    if (rag.slow_list) {                                                                                       \
        const RaggedShardsK *sh = ragged_shards_const(rag.shards) + (f - ragged_const(rag.frames));            \
        const uint32_t n = sh->n, k = (uint32_t)pos.bi % n;                                                    \
        rag.slow_list[ragged_seg_base(f->block0, (uint32_t)f->nbh, (uint32_t)f->nbw, n, k) +                   \
                      atomicAdd(rag.slow_shards + (sh->sh0 + k) * kShardStride, 1u)] = id;                     \
    } else {                                                                                                   \
        rag.fb_list[atomicAdd(rag.fb_count, 1u)] = id;                                                         \
    }
#include "tmfwm_rank1_body.h"
#undef TMF_RANK1_LEFT
}

template <int B>
hipError_t TMF_RAGGED_NAME(embed_rank1_ragged, _b)(const RaggedRank1Args &r, unsigned waves, hipStream_t st)
{
    hipLaunchKernelGGL((TMF_RAGGED_NAME(embed_rank1_ragged, _kernel)<B>), dim3(waves), dim3(64), 0, st, r);
    return hipGetLastError();
}

template hipError_t TMF_RAGGED_NAME(embed_rank1_ragged, _b)<TMF_B>(const RaggedRank1Args &, unsigned, hipStream_t);
#endif

#if TMF_RAGGED_PRE_PART & 2
// The list pass: one wave per shard the chunk uses.  The shard's frame comes from the side
// table's shard prefix (blockIdx.x is wave-uniform: scalar loads, as the strip waves' search), so
// the wave's listed blocks are one frame's and embed_blocks<B, true> runs on that frame's view;
// what it does not certify goes on to fb_list.
template <int B>
__global__ __launch_bounds__(64, kEmbedWaves<B>) void TMF_RAGGED_NAME(embed_ragged, _list_kernel)(RaggedRank1Args r)
{
    constexpr int L = Geo<B>::L, BPW = Geo<B>::BPW, TS = kEmbedTS<B>;
    __shared__ __attribute__((aligned(16))) float lds_all[BPW * TS + kHiPad<B> + kLds2Floats<B>];  // as embed_kernel
    float *lds = lds_all, *lds2 = lds_all + BPW * TS + kHiPad<B>;
    const uint32_t s = blockIdx.x;
    RaggedShardsK *tab = ragged_shards_const(r.shards);
    const int fi = ragged_find(r.nframes, s, [&](int i) { return tab[i].sh0; });
    RaggedFrameK *f = ragged_const(r.frames) + fi;
    const EmbedArgs a = ragged_embed_view<kRaggedAlphas>(r, f);
    const uint32_t block0 = f->block0, nbw = (uint32_t)f->nbw;
    const uint32_t n = r.slow_shards[s * kShardStride];
    const uint32_t base = ragged_seg_base(block0, (uint32_t)f->nbh, nbw, tab[fi].n, s - tab[fi].sh0);
    if (n != 0 && (threadIdx.x & 63) == 0) atomicAdd(r.slow_count, n);
    const int g = (threadIdx.x & 63) / L;
    for (uint32_t t0 = 0; t0 < n; t0 += BPW) {
        StripPos pos;
        pos.valid = t0 + g < n;
        const uint32_t id = pos.valid ? r.slow_list[base + t0 + g] : block0;
        const uint32_t rem = id - block0;
        pos.frame = 0;
        pos.bi = (int)(rem / nbw);
        pos.bj = (int)(rem % nbw);
        embed_blocks<B, true>(a, pos, id, lds, lds2);
        __syncthreads();  // the LDS tiles are reused by the next listed blocks
    }
}

template <int B>
hipError_t TMF_RAGGED_NAME(embed_ragged, _list_b)(const RaggedRank1Args &r, unsigned shards, hipStream_t st)
{
    hipLaunchKernelGGL((TMF_RAGGED_NAME(embed_ragged, _list_kernel)<B>), dim3(shards), dim3(64), 0, st, r);
    return hipGetLastError();
}

template hipError_t TMF_RAGGED_NAME(embed_ragged, _list_b)<TMF_B>(const RaggedRank1Args &, unsigned, hipStream_t);
#endif

}  // namespace tmf
