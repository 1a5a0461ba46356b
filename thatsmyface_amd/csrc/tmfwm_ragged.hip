// Ragged calls (tmfwm_ragged.h): dispatch of the per-size strip and dgesdd-route passes
// (tmfwm_ragged_strip.hip, tmfwm_ragged_fixup.hip) and the ragged edge pass.
#include "tmfwm_passes.h"
#include "tmfwm_ragged.h"

namespace tmf {

#define TMF_RAGGED_DECL(B)                                                                                                   \
    hipError_t launch_embed_ragged_##B(const RaggedArgs &, unsigned, hipStream_t);                                           \
    hipError_t launch_extract_ragged_##B(const RaggedArgs &, unsigned, hipStream_t);                                         \
    hipError_t launch_embed_ragged_fixup_##B(const RaggedArgs &, const uint32_t *, const uint32_t *, int64_t, hipStream_t);  \
    hipError_t launch_extract_ragged_fixup_##B(const RaggedArgs &, const uint32_t *, const uint32_t *, int64_t, hipStream_t);
TMF_RAGGED_DECL(4)
TMF_RAGGED_DECL(6)
TMF_RAGGED_DECL(8)
TMF_RAGGED_DECL(10)
TMF_RAGGED_DECL(12)
TMF_RAGGED_DECL(14)
TMF_RAGGED_DECL(16)

#define TMF_RAGGED_SWITCH(block, call)    \
    switch (block) {                      \
    case 4: return call(4);               \
    case 6: return call(6);               \
    case 8: return call(8);               \
    case 10: return call(10);             \
    case 12: return call(12);             \
    case 14: return call(14);             \
    case 16: return call(16);             \
    default: return hipErrorInvalidValue; \
    }

int ragged_strip_blocks(int block)
{
#define TMF_BPW(B) Geo<B>::BPW
    TMF_RAGGED_SWITCH(block, TMF_BPW)
#undef TMF_BPW
}

// a launch is one workgroup per strip wave: the caller's chunks keep it inside the grid limit
constexpr int64_t kGridMax = 0x7FFFFFFF;

hipError_t launch_embed_ragged(const RaggedArgs &r, int64_t waves, hipStream_t st)
{
    if (waves <= 0 || waves > kGridMax) return hipErrorInvalidValue;
#define TMF_CALL(B) launch_embed_ragged_##B(r, (unsigned)waves, st)
    TMF_RAGGED_SWITCH(r.block, TMF_CALL)
#undef TMF_CALL
}

hipError_t launch_extract_ragged(const RaggedArgs &r, int64_t waves, hipStream_t st)
{
    if (waves <= 0 || waves > kGridMax) return hipErrorInvalidValue;
#define TMF_CALL(B) launch_extract_ragged_##B(r, (unsigned)waves, st)
    TMF_RAGGED_SWITCH(r.block, TMF_CALL)
#undef TMF_CALL
}

hipError_t launch_embed_ragged_fixup(const RaggedArgs &r, const uint32_t *list, const uint32_t *count, int64_t max_entries,
                                     hipStream_t st)
{
#define TMF_CALL(B) launch_embed_ragged_fixup_##B(r, list, count, max_entries, st)
    TMF_RAGGED_SWITCH(r.block, TMF_CALL)
#undef TMF_CALL
}

hipError_t launch_extract_ragged_fixup(const RaggedArgs &r, const uint32_t *list, const uint32_t *count, int64_t max_entries,
                                       hipStream_t st)
{
#define TMF_CALL(B) launch_extract_ragged_fixup_##B(r, list, count, max_entries, st)
    TMF_RAGGED_SWITCH(r.block, TMF_CALL)
#undef TMF_CALL
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
