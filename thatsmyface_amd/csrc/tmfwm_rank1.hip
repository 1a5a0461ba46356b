// The rank-1 pre-pass of the hybrid route (TMFWM_ROUTE_RANK1, round 6), photo mode:
// the single-size kernel and its launch.  The derivation and the constants are in tmfwm_rank1.h,
// the pass's statements in tmfwm_rank1_body.h.
#include "tmfwm_rank1.h"

namespace tmf {

extern template __global__ void embed_kernel<8, true>(EmbedArgs);  // tmfwm_embed8.hip
// the list passes of the other sizes exist for this route only (the hybrid route's strip pass
// there runs every block to the end, kDeferMax<b> = 0): instantiated in tmfwm_rank1_lists.hip
extern template __global__ void embed_kernel<4, true>(EmbedArgs);
extern template __global__ void embed_kernel<6, true>(EmbedArgs);
extern template __global__ void embed_kernel<10, true>(EmbedArgs);
extern template __global__ void embed_kernel<12, true>(EmbedArgs);
extern template __global__ void embed_kernel<14, true>(EmbedArgs);
extern template __global__ void embed_kernel<16, true>(EmbedArgs);

// One wave per strip of the batch: the pre-pass (tmfwm_rank1_body.h) on its blocks.  A block it
// leaves goes to the shard of its row (TMFWM_ROUTE_RANK1: the full hybrid route in the list pass)
// or to the dgesdd-route list (TMFWM_ROUTE_RANK1_REFERENCE: embed_fixup_kernel).
template <int B>
__global__ __launch_bounds__(64, kRank1Waves<B>) void embed_rank1_kernel(EmbedArgs a)
{
    constexpr int L = Geo<B>::L, R = Geo<B>::R, LD = B + 1, NW = Geo<B>::NW;
    constexpr double u53 = 1.1102230246251565e-16;  // 2^-53
    constexpr float u24 = 5.9604644775390625e-08f;  // 2^-24
    __shared__ float lds[kRank1LdsFloats<B>];
    __shared__ uint32_t pix[kRank1PixWords<B>][64];
    const int lane = threadIdx.x & 63, g = lane / L, q = lane % L;
    float *tile = lds + g * B * LD;
    const StripPos pos = strip_pos<B>(a.strips_per_row, a.nbw);
    const uint32_t id = (uint32_t)(((int64_t)blockIdx.y * a.nbh + pos.bi) * a.nbw + pos.bj);
#define TMF_RANK1_LEFT                                                                                         \
    if (a.slow_list) {                                                                                         \
        const uint32_t row = blockIdx.y * (uint32_t)a.nbh + (uint32_t)pos.bi, s = row % kListShards;           \
        a.slow_list[shard_base(s, (uint32_t)a.nframes * (uint32_t)a.nbh, (uint32_t)a.nbw) +                   \
                    atomicAdd(a.slow_shards + s * kShardStride, 1u)] = id;                                     \
    } else {                                                                                                   \
        a.fb_list[atomicAdd(a.fb_count, 1u)] = id;                                                             \
    }
#include "tmfwm_rank1_body.h"
#undef TMF_RANK1_LEFT
}

bool rank1_block(int block) { return block >= 4 && block <= 16 && block % 2 == 0; }

// The rank-1 pre-pass over every block (every slider size, b = 4..16 even), then the edge pixels.  TMFWM_ROUTE_RANK1
// (a.slow_list set): the list pass (embed_kernel<b, true>: the full hybrid route) over the blocks
// it left; TMFWM_ROUTE_RANK1_REFERENCE (no slow list): those blocks went to the dgesdd-route list.
// Either way the caller runs the dgesdd-route fixup next.  The caller handles other block sizes.
hipError_t launch_embed_rank1(EmbedArgs a, hipStream_t st)
{
    if (!rank1_block(a.block)) return hipErrorInvalidValue;
    if (a.nbh > 0 && a.nbw > 0) {
        // TMFWM_ROUTE_RANK1: the list pass over the blocks the pre-pass left
        const hipError_t e = for_block(a.block, [&](auto b) {
            return launch_strips(a, Geo<b()>::BPW, embed_rank1_kernel<b()>, embed_kernel<b(), true>, st);
        });
        if (e != hipSuccess) return e;
    }
    return launch_edges(a.src, a.dst, a.nframes, a.H, a.W, a.frame_stride, a.block, st);
}

}  // namespace tmf
