// Ragged batches (tmfwm_embed_ragged / tmfwm_extract_ragged, and keyed extraction's
// tmfwm_sigma1_map_ragged / tmfwm_extract_keyed_ragged): frames of mixed sizes, each with its own
// buffers, through one set of launches.
//
// The host builds a frame table -- one RaggedFrame per frame, with the exclusive prefix sums of
// the frames' strip waves, blocks and edge pixels -- and uploads it in one copy.  A ragged
// kernel finds its frame by binary search in a prefix, builds the EmbedArgs / ExtractArgs /
// KeyedArgs of that one frame (nframes = 1, strides 0, no list pass) and calls the device function of the
// single-size kernel with it, so a frame's bytes are the single-size path's by construction.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tmfwm_internal.h"

namespace tmf {

struct RaggedFrame {
    const uint8_t *in0;  // embed: the frame's pixels; extract, keyed extract: the watermarked frame; map: the original
    const uint8_t *in1;  // embed: its nbh x nbw tile; extract: the original frame; keyed extract: its nbh x nbw f32 key
                         // (4-byte aligned, read as const float *); map: null
    uint8_t *out;        // embed: the output pixels; extract, keyed extract: the nbh x nbw tile; map: the nbh x nbw
                         // f32 key output (4-byte aligned, written as float *)
    int32_t H, W, nbh, nbw, strips_per_row;
    int32_t aligned;     // as dev_aligned: the pixel buffers (both, or the one of the keyed calls) 4-byte aligned and W % 4 == 0;
                         // keyed calls on 4-byte pixels: the pixel buffer 4-byte aligned, whatever W is
    // exclusive prefix sums over the frames of the chunk (the launches' flat indices):
    uint32_t wave0;      // strip waves, nbh * strips_per_row per frame
    uint32_t block0;     // blocks, nbh * nbw per frame: the block-list ids are block0 + bi * nbw + bj
    int64_t edge0;       // pixels outside the block grid
};
static_assert(sizeof(RaggedFrame) == 64, "frame table entry");

// One alpha per frame (tmfwm_*_ragged_alphas): a side table indexed as `frames` (device memory),
// uploaded with the frame table of each chunk.  A kernel of the per-frame form reads its frame's
// entry where the uniform form reads RaggedArgs::alpha / alpha32; everything else is shared.
struct RaggedAlpha {
    double alpha;   // embed
    float alpha32;  // extract: f32(alpha)
    float pad;
};
static_assert(sizeof(RaggedAlpha) == 16, "alpha table entry");

struct RaggedArgs {
    const RaggedFrame *frames;  // the chunk's frames (device memory)
    int32_t nframes, block;
    double alpha;               // embed
    float alpha32;              // extract: f32(alpha), as ExtractArgs
    uint32_t alphas_off;        // the per-frame form: the chunk's RaggedAlpha entries lie this many bytes behind `frames` (they are
                                // uploaded with the frame table), and the dispatchers take the *_alphas kernels; 0: alpha / alpha32.
                                // (In the struct's padding: the uniform kernels' arguments are where they were.)
    uint32_t *fb_list;          // the dgesdd-route list, ids relative to the chunk, as EmbedArgs / ExtractArgs
    uint32_t *fb_count;
    uint32_t *fb_bad;
};

static_assert(sizeof(RaggedArgs) == 56, "the uniform kernels' argument layout");

// embed with key (tmfwm_embed_key.h): frame i's nbh x nbw f32 key output at keys[i] (device
// memory, indexed as `frames`; 4-byte aligned) -- a side table and an argument struct of this call
// kind's own, so that the frame table keeps its 64-byte entry and the other kinds their arguments
struct RaggedKeyArgs : RaggedArgs {
    float *const *keys;
};

// ---- the list pass of the ragged rank-1 route (TMFWM_ROUTE_RANK1, tmfwm_ragged_pre.hip)
//
// The blocks the ragged pre-pass leaves go to a slow list of the chunk, segmented over the
// kListShards append counters of the single-size list passes (tmfwm_internal.h), but dealt per
// frame: frame i of the chunk owns the shards [sh0, sh0 + n) and its block row bi appends to shard
// sh0 + bi % n, so a list wave (one per shard) holds blocks of one frame and works on that frame's
// one-frame view, wave-uniform as in the strip pass.  A shard's segment of the list starts at
// ragged_seg_base: the frame's own id range [block0, block0 + nbh * nbw) cut at whole rows, so a
// segment's capacity is exactly what its rows can append.
struct RaggedShards {
    uint32_t sh0, n;  // n = 0: a frame without a block (it shares its successor's sh0 and is never found)
};

// a chunk holds at most this many frames with blocks: each needs a shard of its own
inline bool ragged_shards_full(int64_t frames_with_blocks) { return frames_with_blocks >= (int64_t)kListShards; }

// first slot of shard k (0 <= k <= n) of a frame whose nbh rows of nbw blocks are dealt round-robin
// over its n shards (shard k: rows k, k + n, ...)
__host__ __device__ inline uint32_t ragged_seg_base(uint32_t block0, uint32_t nbh, uint32_t nbw, uint32_t n, uint32_t k)
{
    const uint32_t q = nbh / n, r = nbh % n;
    return block0 + (k * q + (k < r ? k : r)) * nbw;
}

// The shard ranges of a chunk's frames f[0 .. n): one shard per frame with blocks, and the
// kListShards - (frames with blocks) left over in proportion to the frames' block rows, at most
// one shard per row.  Returns the shards used (<= kListShards; the caller has kept the chunk to
// kListShards frames with blocks, ragged_shards_full).
template <class Frame>
inline uint32_t ragged_plan_shards(const Frame *f, int64_t n, RaggedShards *out)
{
    uint64_t rows = 0, with_blocks = 0;
    for (int64_t i = 0; i < n; ++i)
        if (f[i].nbh > 0 && f[i].nbw > 0) rows += (uint64_t)f[i].nbh, ++with_blocks;
    const uint64_t spare = (uint64_t)kListShards - with_blocks;
    uint32_t used = 0;
    for (int64_t i = 0; i < n; ++i) {
        uint32_t s = 0;
        if (f[i].nbh > 0 && f[i].nbw > 0) {
            const uint64_t extra = spare * (uint64_t)f[i].nbh / rows, most = (uint64_t)f[i].nbh - 1;
            s = 1 + (uint32_t)(extra < most ? extra : most);
        }
        out[i] = RaggedShards{used, s};
        used += s;
    }
    return used;
}

// the pre-pass and list-pass kernels' arguments: RaggedArgs, the shard side table (indexed as
// `frames`, as RaggedKeyArgs::keys is) and the chunk's slow list (all null on
// TMFWM_ROUTE_RANK1_REFERENCE: a left block goes straight to fb_list)
struct RaggedRank1Args : RaggedArgs {
    const RaggedShards *shards;
    uint32_t *slow_list;
    uint32_t *slow_count;
    uint32_t *slow_shards;
};

// the ragged pre-pass over a chunk's `waves` strip waves, then -- r.slow_list set -- the list pass
// over the `shards` shards the chunk uses
hipError_t launch_embed_rank1_ragged(const RaggedRank1Args &r, int64_t waves, uint32_t shards, hipStream_t st);
template <int B>
hipError_t embed_rank1_ragged_b(const RaggedRank1Args &r, unsigned waves, hipStream_t st);
template <int B>
hipError_t embed_ragged_list_b(const RaggedRank1Args &r, unsigned shards, hipStream_t st);

// blocks per strip wave at this block size (Geo<b>::BPW): the host needs it for strips_per_row
int ragged_strip_blocks(int block);
// strip pass of a chunk: `waves` = the chunk's strip waves (> 0), one workgroup each
hipError_t launch_embed_ragged(const RaggedArgs &r, int64_t waves, hipStream_t st);
hipError_t launch_extract_ragged(const RaggedArgs &r, int64_t waves, hipStream_t st);
// (px: the frames' bytes per pixel, one layout per call -- 3, or 4 for RGBX frames read in place)
hipError_t launch_sigma1_map_ragged(const RaggedArgs &r, int64_t waves, hipStream_t st, int px = 3);
hipError_t launch_extract_keyed_ragged(const RaggedArgs &r, int64_t waves, hipStream_t st, int px = 3);
// embed's key variants: the strip pass and the dgesdd route, each storing its blocks' key entries
hipError_t launch_embed_key_ragged(const RaggedKeyArgs &r, int64_t waves, hipStream_t st);
hipError_t launch_embed_key_ragged_fixup(const RaggedKeyArgs &r, const uint32_t *list, const uint32_t *count, int64_t max_entries,
                                         hipStream_t st);
// colour round trip of the chunk's `pixels` edge pixels (embed)
hipError_t launch_edges_ragged(const RaggedArgs &r, int64_t pixels, hipStream_t st);
// the dgesdd route over the chunk's list (ids as above), max_entries bounds the list
hipError_t launch_embed_ragged_fixup(const RaggedArgs &r, const uint32_t *list, const uint32_t *count, int64_t max_entries,
                                     hipStream_t st);
hipError_t launch_extract_ragged_fixup(const RaggedArgs &r, const uint32_t *list, const uint32_t *count, int64_t max_entries,
                                       hipStream_t st);
hipError_t launch_sigma1_ragged_fixup(const RaggedArgs &r, const uint32_t *list, const uint32_t *count, int64_t max_entries,
                                      hipStream_t st, int px = 3);
hipError_t launch_extract_keyed_ragged_fixup(const RaggedArgs &r, const uint32_t *list, const uint32_t *count, int64_t max_entries,
                                             hipStream_t st, int px = 3);
// the eight launchers per block size B: defined and instantiated for B = TMF_B in the size's own
// translation units (tmfwm_ragged_strip.hip, tmfwm_ragged_fixup.hip), which alone see the kernels
template <int B>
hipError_t embed_ragged_b(const RaggedArgs &r, unsigned waves, hipStream_t st);
template <int B>
hipError_t embed_key_ragged_b(const RaggedKeyArgs &r, unsigned waves, hipStream_t st);
template <int B>
hipError_t embed_key_ragged_fixup_b(const RaggedKeyArgs &r, const uint32_t *list, const uint32_t *count, int64_t max_entries, hipStream_t st);
template <int B>
hipError_t extract_ragged_b(const RaggedArgs &r, unsigned waves, hipStream_t st);
template <int B>
hipError_t embed_ragged_fixup_b(const RaggedArgs &r, const uint32_t *list, const uint32_t *count, int64_t max_entries, hipStream_t st);
template <int B>
hipError_t extract_ragged_fixup_b(const RaggedArgs &r, const uint32_t *list, const uint32_t *count, int64_t max_entries, hipStream_t st);
template <int B>
hipError_t sigma1_map_ragged_b(const RaggedArgs &r, unsigned waves, hipStream_t st, int px);
template <int B>
hipError_t extract_keyed_ragged_b(const RaggedArgs &r, unsigned waves, hipStream_t st, int px);
template <int B>
hipError_t sigma1_ragged_fixup_b(const RaggedArgs &r, const uint32_t *list, const uint32_t *count, int64_t max_entries, hipStream_t st,
                                 int px);
template <int B>
hipError_t extract_keyed_ragged_fixup_b(const RaggedArgs &r, const uint32_t *list, const uint32_t *count, int64_t max_entries,
                                        hipStream_t st, int px);

// The per-frame form (RaggedArgs::alphas_off set): the same sources compiled with
// -DTMF_RAGGED_ALPHAS=1 into objects of their own (the Makefile's ALPHA_OBJS), whose kernels and
// launchers carry _alphas in their names -- embed_ragged_alphas_kernel<b> beside
// embed_ragged_kernel<b>, as the px4 kernels stand beside the 3-byte ones.  No uniform kernel
// shares a translation unit with a new one, so its code is the parent's: the inliner counts a
// function's call sites per unit, and a second kernel calling embed_blocks<b> costs
// embed_ragged_kernel<6> a wave per SIMD (profiles/ragged_alphas).  The map takes no alpha.
#ifndef TMF_RAGGED_ALPHAS
#define TMF_RAGGED_ALPHAS 0
#endif
#if TMF_RAGGED_ALPHAS
#define TMF_RAGGED_NAME(stem, rest) stem##_alphas##rest
#else
#define TMF_RAGGED_NAME(stem, rest) stem##rest
#endif
template <int B>
hipError_t embed_ragged_alphas_b(const RaggedArgs &r, unsigned waves, hipStream_t st);
template <int B>
hipError_t embed_key_ragged_alphas_b(const RaggedKeyArgs &r, unsigned waves, hipStream_t st);
template <int B>
hipError_t extract_ragged_alphas_b(const RaggedArgs &r, unsigned waves, hipStream_t st);
template <int B>
hipError_t extract_keyed_ragged_alphas_b(const RaggedArgs &r, unsigned waves, hipStream_t st, int px);
template <int B>
hipError_t embed_ragged_alphas_fixup_b(const RaggedArgs &r, const uint32_t *list, const uint32_t *count, int64_t max_entries, hipStream_t st);
template <int B>
hipError_t embed_key_ragged_alphas_fixup_b(const RaggedKeyArgs &r, const uint32_t *list, const uint32_t *count, int64_t max_entries,
                                           hipStream_t st);
template <int B>
hipError_t extract_ragged_alphas_fixup_b(const RaggedArgs &r, const uint32_t *list, const uint32_t *count, int64_t max_entries, hipStream_t st);
template <int B>
hipError_t extract_keyed_ragged_alphas_fixup_b(const RaggedArgs &r, const uint32_t *list, const uint32_t *count, int64_t max_entries,
                                               hipStream_t st, int px);
template <int B>
hipError_t embed_rank1_ragged_alphas_b(const RaggedRank1Args &r, unsigned waves, hipStream_t st);
template <int B>
hipError_t embed_ragged_alphas_list_b(const RaggedRank1Args &r, unsigned shards, hipStream_t st);

#if defined(__HIPCC__)
// The table through the constant address space: a load from it at a wave-uniform address is a
// scalar load, so what a strip wave reads of its frame stays in SGPRs (the VGPR budget of
// embed_blocks is spent to the last register, tmfwm_blocks.h).
#define TMF_CONST_AS __attribute__((address_space(4)))
using RaggedFrameK = const TMF_CONST_AS RaggedFrame;
__device__ __forceinline__ RaggedFrameK *ragged_const(const RaggedFrame *p) { return (RaggedFrameK *)p; }
// the key side table the same way (RaggedKeyArgs::keys)
using RaggedKeyK = float *const TMF_CONST_AS;
__device__ __forceinline__ RaggedKeyK *ragged_key_const(float *const *p) { return (RaggedKeyK *)p; }
// and the shard side table (RaggedRank1Args::shards)
using RaggedShardsK = const TMF_CONST_AS RaggedShards;
__device__ __forceinline__ RaggedShardsK *ragged_shards_const(const RaggedShards *p) { return (RaggedShardsK *)p; }
// and the alpha side table (RaggedArgs::alphas_off)
using RaggedAlphaK = const TMF_CONST_AS RaggedAlpha;

// Frame f's entry of the alpha table, in f's address space: a strip, pre-pass or list wave holds
// its frame in the constant address space (wave-uniform: a scalar load), a fixup lane the frame of
// its listed block in the generic one (a wave holds blocks of several frames).
__device__ __forceinline__ RaggedAlphaK *ragged_alpha_entry(const RaggedArgs &r, RaggedFrameK *f)
{
    return (RaggedAlphaK *)((const TMF_CONST_AS uint8_t *)ragged_const(r.frames) + r.alphas_off) + (f - ragged_const(r.frames));
}
__device__ __forceinline__ const RaggedAlpha *ragged_alpha_entry(const RaggedArgs &r, const RaggedFrame *f)
{
    return (const RaggedAlpha *)((const uint8_t *)r.frames + r.alphas_off) + (f - r.frames);
}

// the frame that owns flat index x: the last i in [0, n) with prefix(i) <= x (frames with
// nothing to do share their successor's prefix and are never found)
template <class Prefix>
__device__ __forceinline__ int ragged_find(int n, uint64_t x, Prefix prefix)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((uint64_t)prefix(mid) <= x) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// the one-frame views of frame f (a table entry in either address space); PF: the per-frame form,
// the frame's alpha from the alpha table.  The form is a template argument of every view and of
// every helper between a kernel and its view -- a unit's kernels pass kRaggedAlphas -- so the two
// forms of a helper are two functions by name, never one name with two bodies.
constexpr bool kRaggedAlphas = TMF_RAGGED_ALPHAS != 0;
template <bool PF, class F>
__device__ __forceinline__ EmbedArgs ragged_embed_view(const RaggedArgs &r, F *f)
{
    EmbedArgs a;
    a.src = f->in0;
    a.dst = f->out;
    a.wm = f->in1;
    a.wm_stride = 0;
    a.nframes = 1;
    a.frame_stride = 0;
    a.H = f->H;
    a.W = f->W;
    a.block = r.block;
    a.nbh = f->nbh;
    a.nbw = f->nbw;
    a.strips_per_row = f->strips_per_row;
    a.aligned = f->aligned;
    if constexpr (PF) a.alpha = ragged_alpha_entry(r, f)->alpha;
    else a.alpha = r.alpha;
    a.fb_list = r.fb_list;
    a.fb_count = r.fb_count;
    a.fb_bad = r.fb_bad;
    a.slow_list = nullptr;  // no list pass: the strip pass runs every block to the end
    a.slow_count = nullptr;
    a.slow_shards = nullptr;
    a.key_out = nullptr;    // the key variants set it from RaggedKeyArgs::keys
    a.key_stride = 0;
    return a;
}

template <bool PF, class F>
__device__ __forceinline__ ExtractArgs ragged_extract_view(const RaggedArgs &r, F *f)
{
    ExtractArgs a;
    a.wsrc = f->in0;
    a.osrc = f->in1;
    a.out = f->out;
    a.nframes = 1;
    a.frame_stride = 0;
    a.tile_stride = 0;
    a.H = f->H;
    a.W = f->W;
    a.block = r.block;
    a.nbh = f->nbh;
    a.nbw = f->nbw;
    a.strips_per_row = f->strips_per_row;
    a.aligned = f->aligned;
    if constexpr (PF) a.alpha32 = ragged_alpha_entry(r, f)->alpha32;
    else a.alpha32 = r.alpha32;
    a.fb_list = r.fb_list;
    a.fb_count = r.fb_count;
    a.fb_bad = r.fb_bad;
    a.slow_list = nullptr;  // undecided blocks go straight to the dgesdd route
    a.slow_count = nullptr;
    a.slow_shards = nullptr;
    return a;
}

// keyed extraction: one image per frame; in1 is the key (keyed extract), out the key output (map) or the tile
template <bool PF, class F>
__device__ __forceinline__ KeyedArgs ragged_keyed_view(const RaggedArgs &r, F *f)
{
    KeyedArgs a;
    a.src = f->in0;
    a.key = (const float *)f->in1;
    a.key_out = (float *)f->out;
    a.out = f->out;
    a.nframes = 1;
    a.frame_stride = 0;
    a.tile_stride = 0;
    a.key_stride = 0;
    a.H = f->H;
    a.W = f->W;
    a.block = r.block;
    a.nbh = f->nbh;
    a.nbw = f->nbw;
    a.strips_per_row = f->strips_per_row;
    a.aligned = f->aligned;
    if constexpr (PF) a.alpha32 = ragged_alpha_entry(r, f)->alpha32;
    else a.alpha32 = r.alpha32;
    a.fb_list = r.fb_list;
    a.fb_count = r.fb_count;
    a.fb_bad = r.fb_bad;
    a.slow_list = nullptr;  // undecided blocks go straight to the dgesdd route
    a.slow_count = nullptr;
    a.slow_shards = nullptr;
    return a;
}
#endif

}  // namespace tmf
