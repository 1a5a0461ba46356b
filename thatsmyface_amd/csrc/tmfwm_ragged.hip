// Ragged calls (tmfwm_ragged.h): dispatch of the per-size strip and dgesdd-route passes
// (tmfwm_ragged_strip.hip, tmfwm_ragged_fixup.hip) and the ragged edge pass.
#include "tmfwm_passes.h"
#include "tmfwm_ragged.h"

namespace tmf {

int ragged_strip_blocks(int block)
{
    return block_value(block, 1, [](auto b) { return (int)Geo<b()>::BPW; });  // (the callers have checked the size)
}

// (r.alphas_off set: the per-frame form, the *_alphas launchers of the units built with -DTMF_RAGGED_ALPHAS=1)
//
// a launch is one workgroup per strip wave: the caller's chunks keep it inside the grid limit
constexpr int64_t kGridMax = 0x7FFFFFFF;

hipError_t launch_embed_ragged(const RaggedArgs &r, int64_t waves, hipStream_t st)
{
    if (waves <= 0 || waves > kGridMax) return hipErrorInvalidValue;
    return for_block(r.block, [&](auto b) { return r.alphas_off ? embed_ragged_alphas_b<b()>(r, (unsigned)waves, st) : embed_ragged_b<b()>(r, (unsigned)waves, st); });
}

hipError_t launch_embed_rank1_ragged(const RaggedRank1Args &r, int64_t waves, uint32_t shards, hipStream_t st)
{
    if (waves <= 0 || waves > kGridMax || shards > kListShards || (r.slow_list && shards == 0)) return hipErrorInvalidValue;
    return for_block(r.block, [&](auto b) {
        const bool pf = r.alphas_off != 0;
        const hipError_t e = pf ? embed_rank1_ragged_alphas_b<b()>(r, (unsigned)waves, st) : embed_rank1_ragged_b<b()>(r, (unsigned)waves, st);
        if (e != hipSuccess || !r.slow_list) return e;
        return pf ? embed_ragged_alphas_list_b<b()>(r, shards, st) : embed_ragged_list_b<b()>(r, shards, st);
    });
}

hipError_t launch_embed_key_ragged(const RaggedKeyArgs &r, int64_t waves, hipStream_t st)
{
    if (waves <= 0 || waves > kGridMax) return hipErrorInvalidValue;
    return for_block(r.block, [&](auto b) { return r.alphas_off ? embed_key_ragged_alphas_b<b()>(r, (unsigned)waves, st) : embed_key_ragged_b<b()>(r, (unsigned)waves, st); });
}

hipError_t launch_embed_key_ragged_fixup(const RaggedKeyArgs &r, const uint32_t *list, const uint32_t *count, int64_t max_entries,
                                         hipStream_t st)
{
    return for_block(r.block, [&](auto b) {
        return r.alphas_off ? embed_key_ragged_alphas_fixup_b<b()>(r, list, count, max_entries, st)
                            : embed_key_ragged_fixup_b<b()>(r, list, count, max_entries, st);
    });
}

hipError_t launch_extract_ragged(const RaggedArgs &r, int64_t waves, hipStream_t st)
{
    if (waves <= 0 || waves > kGridMax) return hipErrorInvalidValue;
    return for_block(r.block, [&](auto b) { return r.alphas_off ? extract_ragged_alphas_b<b()>(r, (unsigned)waves, st) : extract_ragged_b<b()>(r, (unsigned)waves, st); });
}

hipError_t launch_sigma1_map_ragged(const RaggedArgs &r, int64_t waves, hipStream_t st, int px)
{
    if (waves <= 0 || waves > kGridMax || (px != 3 && px != 4)) return hipErrorInvalidValue;
    return for_block(r.block, [&](auto b) { return sigma1_map_ragged_b<b()>(r, (unsigned)waves, st, px); });
}

hipError_t launch_extract_keyed_ragged(const RaggedArgs &r, int64_t waves, hipStream_t st, int px)
{
    if (waves <= 0 || waves > kGridMax || (px != 3 && px != 4)) return hipErrorInvalidValue;
    return for_block(r.block, [&](auto b) {
        return r.alphas_off ? extract_keyed_ragged_alphas_b<b()>(r, (unsigned)waves, st, px) : extract_keyed_ragged_b<b()>(r, (unsigned)waves, st, px);
    });
}

hipError_t launch_embed_ragged_fixup(const RaggedArgs &r, const uint32_t *list, const uint32_t *count, int64_t max_entries,
                                     hipStream_t st)
{
    return for_block(r.block, [&](auto b) {
        return r.alphas_off ? embed_ragged_alphas_fixup_b<b()>(r, list, count, max_entries, st) : embed_ragged_fixup_b<b()>(r, list, count, max_entries, st);
    });
}

hipError_t launch_extract_ragged_fixup(const RaggedArgs &r, const uint32_t *list, const uint32_t *count, int64_t max_entries,
                                       hipStream_t st)
{
    return for_block(r.block, [&](auto b) {
        return r.alphas_off ? extract_ragged_alphas_fixup_b<b()>(r, list, count, max_entries, st)
                            : extract_ragged_fixup_b<b()>(r, list, count, max_entries, st);
    });
}

hipError_t launch_sigma1_ragged_fixup(const RaggedArgs &r, const uint32_t *list, const uint32_t *count, int64_t max_entries,
                                      hipStream_t st, int px)
{
    if (px != 3 && px != 4) return hipErrorInvalidValue;
    return for_block(r.block, [&](auto b) { return sigma1_ragged_fixup_b<b()>(r, list, count, max_entries, st, px); });
}

hipError_t launch_extract_keyed_ragged_fixup(const RaggedArgs &r, const uint32_t *list, const uint32_t *count, int64_t max_entries,
                                             hipStream_t st, int px)
{
    if (px != 3 && px != 4) return hipErrorInvalidValue;
    return for_block(r.block, [&](auto b) {
        return r.alphas_off ? extract_keyed_ragged_alphas_fixup_b<b()>(r, list, count, max_entries, st, px)
                            : extract_keyed_ragged_fixup_b<b()>(r, list, count, max_entries, st, px);
    });
}

// The edge pixels of every frame of the chunk on one flat index over the table's edge prefix;
// a frame without a full block is all edge.  The per-pixel work is edge_roundtrip_kernel's.
__global__ __launch_bounds__(256) void edge_ragged_kernel(RaggedArgs r, int64_t pixels)
{
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= pixels) return;
    const RaggedFrame *f = r.frames + ragged_find(r.nframes, (uint64_t)idx, [&](int i) { return r.frames[i].edge0; });
    EdgeArgs e;
    e.src = f->in0;
    e.dst = f->out;
    e.frame_stride = 0;
    e.H = f->H;
    e.W = f->W;
    e.core_h = f->nbh * r.block;
    e.core_w = f->nbw * r.block;
    e.edge_w = e.W - e.core_w;
    edge_roundtrip_pixel(e, idx - f->edge0, 0);
}

hipError_t launch_edges_ragged(const RaggedArgs &r, int64_t pixels, hipStream_t st)
{
    if (pixels <= 0) return hipSuccess;
    const int64_t grid = (pixels + 255) / 256;
    if (grid > kGridMax) return hipErrorInvalidValue;
    hipLaunchKernelGGL(edge_ragged_kernel, dim3((unsigned)grid), dim3(256), 0, st, r, pixels);
    return hipGetLastError();
}

}  // namespace tmf
