// Internal launch interface between the C-ABI (tmfwm_capi.cpp) and the kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/tmfwm.h"
#include "tmfwm_sizes.h"
#include "tmfwm_tile_plan.h"

namespace tmf {

// One append counter per segment instead of one per launch: at b = 4 most strip-pass waves
// append, and device-scope atomics on one address serialise.
constexpr uint32_t kListShards = 2048, kShardStride = 16;  // counters 64 bytes apart

// first slot of segment s when rows block rows of nbw blocks are dealt round-robin over
// kListShards segments (segment s holds rows s, s + kListShards, ...; exact capacity)
__host__ __device__ inline uint32_t shard_base(uint32_t s, uint32_t rows, uint32_t nbw)
{
    const uint32_t q = rows / kListShards, r = rows % kListShards;
    return (uint32_t)(((uint64_t)s * q + (s < r ? s : r)) * nbw);
}

struct EmbedArgs {
    const uint8_t *src;
    uint8_t *dst;
    const uint8_t *wm;       // nbh x nbw tile of frame 0
    int64_t wm_stride;       // bytes between consecutive frames' tiles; 0: one tile shared by all frames
    int64_t nframes;
    int64_t frame_stride;    // bytes between frames (>= H*W*3)
    int H, W, block, nbh, nbw, strips_per_row;
    int aligned;             // 4-byte aligned pixel rows: dword loads/stores
    double alpha;
    // blocks the conditioning test sends to the dgesdd route: ids (frame * nbh + bi) * nbw + bj
    // relative to this launch, appended at fb_list[atomicAdd(fb_count, 1)]
    uint32_t *fb_list;
    uint32_t *fb_count;
    uint32_t *fb_bad;        // dgesdd-route blocks whose dbdsqr did not converge (may be null)
    // list pass: blocks the first pass leaves unfinished after its f64 sweep
    // budget, same ids; null: the first pass runs every block to the end.  Segmented as
    // ExtractArgs' list (kListShards, shard_base, slow_shards)
    uint32_t *slow_list;
    uint32_t *slow_count;
    uint32_t *slow_shards;
    // the key variants of the embed kernels (tmfwm_embed_key.h) store f32(sigma_1) of
    // every block of `src` here, as sigma1_map does: nframes x (nbh x nbw) f32, key_stride floats
    // apart.  Null / 0 in every other call (the plain kernels never read them).
    float *key_out;
    int64_t key_stride;
};

struct ExtractArgs {
    const uint8_t *wsrc;
    const uint8_t *osrc;
    uint8_t *out;            // nframes x (nbh x nbw), tile_stride bytes apart
    int64_t nframes;
    int64_t frame_stride;
    int64_t tile_stride;
    int H, W, block, nbh, nbw, strips_per_row;
    int aligned;
    float alpha32;           // f32(alpha): numpy-2 weak-scalar promotion (watermarking.py:285)
    uint32_t *fb_list;       // blocks whose sigma_1 enclosure is undecided (dgesdd route)
    uint32_t *fb_count;
    uint32_t *fb_bad;        // dgesdd-route blocks whose dbdsqr did not converge (may be null)
    // list pass: blocks the strip pass's power iterations left undecided, redone
    // with more iterations before the dgesdd route; null: straight to the dgesdd route.  The
    // list is kListShards segments (shard_base); block row r = frame * nbh + bi appends to
    // segment r % kListShards through its own counter slow_shards[s * kShardStride] (zeroed by
    // the caller); the list pass adds the segments' lengths into *slow_count.
    uint32_t *slow_list;
    uint32_t *slow_count;
    uint32_t *slow_shards;
};

// Keyed extraction (tmfwm_keyed.hip): one image per frame.  The map pass stores
// f32(sigma_1) of every block of `src` into key_out; the keyed extract reads the original's
// sigma_1 from `key` instead of recomputing it from the original's pixels.
struct KeyedArgs {
    const uint8_t *src;      // map: the original frames; extract: the watermarked frames
    const float *key;        // extract: nbh x nbw f32 per frame, key_stride floats apart (0: one key for all frames)
    float *key_out;          // map: nframes x (nbh x nbw) f32, key_stride floats apart
    uint8_t *out;            // extract: nframes x (nbh x nbw), tile_stride bytes apart
    int64_t nframes;
    int64_t frame_stride;
    int64_t tile_stride;
    int64_t key_stride;      // in floats
    int H, W, block, nbh, nbw, strips_per_row;
    int aligned;             // 3-byte pixels: as ExtractArgs; 4-byte pixels: src and frame_stride are multiples of 4
    float alpha32;
    // the lists and counters of ExtractArgs, used the same way
    uint32_t *fb_list;
    uint32_t *fb_count;
    uint32_t *fb_bad;
    uint32_t *slow_list;
    uint32_t *slow_count;
    uint32_t *slow_shards;
};

struct EdgeArgs {
    const uint8_t *src;
    uint8_t *dst;
    int64_t frame_stride;
    int H, W, core_h, core_w, edge_w;
};

// error reporting and argument checks of the C ABI (tmfwm_capi.cpp), shared with tmfwm_multi.cpp
int report(int code, const char *fmt, ...);  // sets this thread's tmfwm_last_error(); returns code
void clear_error();
int check_frames(int64_t n, int32_t H, int32_t W, int64_t stride, int32_t block);

// Device-memory embed / extract that never synchronise (tmfwm_multi.cpp's pipelined passes).
// Instead of reading the per-chunk counts back, they go to `sink` -- pinned host memory of
// 3 * count_chunks(...) uint32 entries: the chunks' dgesdd-route counts, then their dbdsqr
// non-convergence counts, then their list-pass counts -- by a copy enqueued on the stream; the
// caller sums them with sum_sink() once the stream is done.  Arguments as tmfwm_embed_ex /
// tmfwm_extract_ex with TMFWM_MEM_DEVICE (checked the same way).
int64_t count_chunks(int64_t nframes, int H, int W, int block);
// embed: frame f's tile at tile + f * tile_stride (0: one tile shared by all frames)
int embed_device_async(const uint8_t *src, int64_t n, int H, int W, int64_t stride, const uint8_t *tile, int64_t tile_stride,
                       int block, double alpha, uint8_t *dst, hipStream_t st, uint32_t *sink, int route = TMFWM_ROUTE_HYBRID);
int extract_device_async(const uint8_t *wsrc, const uint8_t *osrc, int64_t n, int H, int W, int64_t stride, int block,
                         double alpha, uint8_t *out, hipStream_t st, uint32_t *sink, int route = TMFWM_ROUTE_HYBRID);
int sum_sink(const uint32_t *sink, int64_t nchunks, int64_t *lapack);  // TMFWM_ERR_HIP on non-convergence

// ---- launch shapes shared by the launchers (host side)

// A grid's y dimension takes at most 65535 frames.  The C ABI's chunks never hold more
// (tmfwm_capi.cpp, Chunks::plan), and the strip launchers refuse more: a listed block's id is
// relative to its launch, so a chunk cut into several strip launches would hand its list pass ids
// of the wrong frames.  Launches that keep no list (edge pixels, synthetic frames) are cut here.
constexpr int64_t kMaxGridY = 65535;

// launch(f0, nf) for frames [f0, f0 + nf) in slices of at most kMaxGridY frames
template <class Launch>
inline hipError_t for_frame_slices(int64_t nframes, Launch launch)
{
    for (int64_t f0 = 0; f0 < nframes; f0 += kMaxGridY) launch(f0, nframes - f0 < kMaxGridY ? nframes - f0 : kMaxGridY);
    return hipGetLastError();
}

// the list pass's grid: one wave per segment that can hold a block row (the others stay empty)
inline unsigned list_grid(int64_t rows) { return (unsigned)(rows < (int64_t)kListShards ? rows : (int64_t)kListShards); }

// The strip pass of a chunk -- one wave per strip of bpw blocks, frames on the grid's y -- and
// then, if the chunk has one (`list` and a.slow_list set), the list pass over what it deferred.
template <class Args>
inline hipError_t launch_strips(Args a, int bpw, void (*strip)(Args), void (*list)(Args), hipStream_t st)
{
    if (a.nframes > kMaxGridY) return hipErrorInvalidValue;
    a.strips_per_row = (a.nbw + bpw - 1) / bpw;
    hipLaunchKernelGGL(strip, dim3((unsigned)((int64_t)a.strips_per_row * a.nbh), (unsigned)a.nframes), dim3(64), 0, st, a);
    if (list && a.slow_list) hipLaunchKernelGGL(list, dim3(list_grid(a.nframes * a.nbh)), dim3(64), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_embed(const EmbedArgs &a, hipStream_t st);  // a.key_out set: the key variants (tmfwm_embed_key.hip)
hipError_t launch_embed_key_strips(const EmbedArgs &a, hipStream_t st);
bool embed_key_fused(int block);  // the key comes out of the embed passes at this size (tmfwm_embed_key.h)
hipError_t launch_embed_rank1(EmbedArgs a, hipStream_t st);  // TMFWM_ROUTE_RANK1 (tmfwm_rank1.hip)
bool rank1_block(int block);  // the block sizes TMFWM_ROUTE_RANK1 has a pre-pass for
bool embed_defers(int block);  // the strip pass of embed_kernel<block> can leave blocks to a list pass
hipError_t launch_edges(const uint8_t *src, uint8_t *dst, int64_t nframes, int H, int W, int64_t frame_stride, int block, hipStream_t st);
hipError_t launch_extract(const ExtractArgs &a, hipStream_t st);
hipError_t launch_rgb_to_ycbcr(const uint8_t *rgb, int64_t npix, float *ycc, hipStream_t st);
hipError_t launch_rgb_to_ycbcr_f32(const float *rgb, int64_t npix, float *ycc, hipStream_t st);
hipError_t launch_ycbcr_to_rgb(const void *ycc, int dtype, int64_t npix, uint8_t *rgb, hipStream_t st); // dtype TMFWM_DT_F16/F32/F64
hipError_t launch_dct2d_blocks(float *blocks, int64_t nb, int block, int inverse, hipStream_t st);
// second pass on the dgesdd route (tmfwm_fallback.hip); max_entries bounds the list
hipError_t launch_embed_fixup(const EmbedArgs &a, const uint32_t *list, const uint32_t *count, int64_t max_entries, hipStream_t st);
hipError_t launch_extract_fixup(const ExtractArgs &a, const uint32_t *list, const uint32_t *count, int64_t max_entries, hipStream_t st);
// their launchers per block size B: declared here, defined and instantiated for B = TMF_B in the
// size's own translation unit (tmfwm_fixup.hip, tmfwm_keyed_fixup.hip), which alone sees the kernels
template <int B>
hipError_t embed_fixup_b(const EmbedArgs &a, const uint32_t *list, const uint32_t *count, int64_t max_entries, hipStream_t st);
template <int B>
hipError_t embed_key_fixup_b(const EmbedArgs &a, const uint32_t *list, const uint32_t *count, int64_t max_entries, hipStream_t st);
template <int B>
hipError_t embed_key_strips_b(const EmbedArgs &a, hipStream_t st);  // tmfwm_embed_key.hip
template <int B>
hipError_t extract_fixup_b(const ExtractArgs &a, const uint32_t *list, const uint32_t *count, int64_t max_entries, hipStream_t st);
template <int B>
hipError_t sigma1_fixup_b(const KeyedArgs &a, const uint32_t *list, const uint32_t *count, int64_t max_entries, hipStream_t st, int px);
template <int B>
hipError_t extract_keyed_fixup_b(const KeyedArgs &a, const uint32_t *list, const uint32_t *count, int64_t max_entries, hipStream_t st,
                                 int px);
// keyed extraction (tmfwm_keyed.hip; the dgesdd-route passes per block size: tmfwm_keyed_fixup.hip).
// px: bytes per pixel of the frames at a.src -- 3, or 4 (R G B pad) for the kernels that read
// RGBX frames in place; a.aligned then means base and frame stride are multiples of 4
hipError_t launch_sigma1_map(const KeyedArgs &a, hipStream_t st, int px = 3);
hipError_t launch_extract_keyed(const KeyedArgs &a, hipStream_t st, int px = 3);
hipError_t launch_sigma1_fixup(const KeyedArgs &a, const uint32_t *list, const uint32_t *count, int64_t max_entries, hipStream_t st,
                               int px = 3);
hipError_t launch_extract_keyed_fixup(const KeyedArgs &a, const uint32_t *list, const uint32_t *count, int64_t max_entries,
                                      hipStream_t st, int px = 3);
// the reference route: list = 0 .. n-1, *count = n (every block of a launch on the dgesdd route)
hipError_t launch_list_all(uint32_t *list, uint32_t *count, int64_t n, hipStream_t st);
// RGBX (4 bytes per pixel, PIL's in-memory "RGB") <-> RGB (3 bytes) per frame (tmfwm_pixels.hip);
// strides in bytes between frames; unpack writes 255 into the pad byte
hipError_t launch_pack_rgbx(const uint8_t *src4, int64_t sstride, uint8_t *dst3, int64_t dstride, int64_t n, int H, int W,
                            hipStream_t st);
hipError_t launch_unpack_rgbx(const uint8_t *src3, int64_t sstride, uint8_t *dst4, int64_t dstride, int64_t n, int H, int W,
                              hipStream_t st);
hipError_t launch_lapack_svd_blocks(const float *D, int64_t nb, int block, float *U, float *S, float *Vt, int want_v, int32_t *info,
                                    hipStream_t st);
hipError_t launch_lapack_nrm2(const double *x, int64_t nvec, int n, int inc, double *out, hipStream_t st);
hipError_t launch_svd_blocks(const float *D, int64_t nb, int block, float *U, float *S, float *Vt, int32_t *sweeps, hipStream_t st);
// Watermark-tile preparation (tmfwm_tile.hip): Pillow's LANCZOS resample tables (ResampleAxis:
// tmfwm_tile_plan.h).
struct ResamplePlan {
    int ih = 0, iw = 0, oh = 0, ow = 0, y_first = 0, y_last = 0;
    bool need_h = false, need_v = false;
    ResampleAxis h, v;
    void build(int in_h, int in_w, int out_h, int out_w);
    int rows() const { return y_last - y_first; }
    size_t tmp_bytes() const { return need_h ? (size_t)rows() * ow : 0; }
    std::vector<int> pack() const;  // [bounds_h | kk_h | bounds_v | kk_v]
};

hipError_t launch_resize_lanczos(const uint8_t *in, const ResamplePlan &plan, const int *tables, uint8_t *tmp, uint8_t *out,
                                 int ldo, hipStream_t st);
// n equally sized images in_stride bytes apart -> n outputs out_stride bytes apart, one plan and
// one table upload for all of them; tmp: device scratch of resize_tmp_bytes(plan, n)
constexpr int64_t kResizeGroup = 1024;  // images per launch
size_t resize_tmp_bytes(const ResamplePlan &plan, int64_t n);
hipError_t launch_resize_lanczos_batch(const uint8_t *in, int64_t in_stride, int64_t n, const ResamplePlan &plan, const int *tables,
                                       uint8_t *tmp, uint8_t *out, int ldo, int64_t out_stride, hipStream_t st);
// One group of a ragged call (tmfwm_tile_plan.h): jobs [0, n) of the group in device memory, the
// call's packed tables, the shared scratch; the horizontal launch only where h_items > 0.
hipError_t launch_tiles_ragged(const TileJob *jobs, int64_t n, const int *tables, uint8_t *scratch, int64_t h_items,
                               int64_t v_items, hipStream_t st);
hipError_t launch_synth(uint64_t seed, int64_t frame0, int64_t nframes, int64_t frame_bytes, uint8_t *out, hipStream_t st);

}  // namespace tmf
