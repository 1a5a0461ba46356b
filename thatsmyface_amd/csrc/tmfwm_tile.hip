// Watermark-tile preparation on the GPU: resize_watermark (watermarking.py:102-132)
// after the host's PNG decode + convert("L").  Pillow 12.2.0's Image.resize(LANCZOS)
// on an 8-bit image (Resample.c) is two integer passes over 22-bit fixed-point
// coefficients: a horizontal pass over the source rows the vertical filter uses,
// then a vertical pass; preserve_ratio pastes the result centred on a white canvas.
//
// The coefficient tables are built on the host here (double precision, the same
// libm sin() Pillow calls, so the rounding to fixed point is Pillow's), uploaded
// once per call, and the passes run as kernels -- one thread per output byte.  The
// tile is tiny (<= 480 x 270 for a 4K frame at b = 8); doing it on the device lets
// a multi-GPU job build the broadcast tile where it is consumed, without PIL.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <vector>

#include "tmfwm_internal.h"
#include "tmfwm_ragged.h"  // TMF_CONST_AS

namespace tmf {

// The three kernels take the image index from blockIdx.z: image i is read at in + i * istride
// and written at out + i * ostride (one launch over a batch of equally sized images).
//
// out[yy][xx] = clip8(2^21 + sum_x in[yy + y0][xmin + x] * k[xx][x])
__global__ __launch_bounds__(256) void resample_h_kernel(const uint8_t *__restrict__ in, int64_t istride, int iw, int y0, int rows,
                                                         int ow, const int *__restrict__ bounds, const int *__restrict__ kk, int ks,
                                                         uint8_t *__restrict__ out, int64_t ostride, int ldo)
{
    const int xx = blockIdx.x * blockDim.x + threadIdx.x, yy = blockIdx.y;
    if (xx >= ow || yy >= rows) return;
    in += blockIdx.z * istride;
    out += blockIdx.z * ostride;
    const int xmin = bounds[2 * xx], xmax = bounds[2 * xx + 1];
    const uint8_t *src = in + (int64_t)(yy + y0) * iw + xmin;
    const int *k = kk + (int64_t)xx * ks;
    out[(int64_t)yy * ldo + xx] = resample_h_byte(src, k, xmax);
}

// out[yy][xx] = clip8(2^21 + sum_y in[ymin + y][xx] * k[yy][y])
__global__ __launch_bounds__(256) void resample_v_kernel(const uint8_t *__restrict__ in, int64_t istride, int iw, int oh,
                                                         const int *__restrict__ bounds, const int *__restrict__ kk, int ks,
                                                         uint8_t *__restrict__ out, int64_t ostride, int ldo)
{
    const int xx = blockIdx.x * blockDim.x + threadIdx.x, yy = blockIdx.y;
    if (xx >= iw || yy >= oh) return;
    in += blockIdx.z * istride;
    out += blockIdx.z * ostride;
    const int ymin = bounds[2 * yy], ymax = bounds[2 * yy + 1];
    const int *k = kk + (int64_t)yy * ks;
    out[(int64_t)yy * ldo + xx] = resample_v_byte(in, iw, xx, ymin, k, ymax);
}

__global__ __launch_bounds__(256) void copy_rows_kernel(const uint8_t *__restrict__ in, int64_t istride, int iw, int rows,
                                                        uint8_t *__restrict__ out, int64_t ostride, int ldo)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x < iw && y < rows) out[blockIdx.z * ostride + (int64_t)y * ldo + x] = in[blockIdx.z * istride + (int64_t)y * iw + x];
}

// ---- the ragged call (tmfwm_prepare_tiles_ragged; the plan and the per-thread bodies: tmfwm_tile_plan.h)
//
// Both grids are flat: one workgroup of kTileSeg threads -- one wave -- per row segment of the
// group's jobs.  The wave finds its job by binary search in the work-item prefix of the job table,
// read through the constant address space: the job's fields are scalar loads and stay in SGPRs.

// The intermediate rows [y_first, y_first + rows) x rw of every job with need_h, into the scratch.
// The taps differ per thread (one output column each), so the tables are ordinary global loads.
__global__ __launch_bounds__(kTileSeg) void resample_h_ragged_kernel(const TileJob *jobs, int n, const int *__restrict__ tables,
                                                                     uint8_t *__restrict__ scratch)
{
    const TMF_CONST_AS TileJob *J = (const TMF_CONST_AS TileJob *)jobs;
    const uint32_t item = blockIdx.x;
    const int j = tile_find(n, item, [&](int i) { return J[i].h_item0; });
    tile_h_thread(J + j, item - J[j].h_item0, (int)threadIdx.x, tables, scratch);
}

// Every byte of every tile: 255 outside the paste rectangle, the vertical taps (or a copy) inside.
// Job and output row are the wave's, so a row's bounds and taps come through scalar loads too.
__global__ __launch_bounds__(kTileSeg) void resample_v_paste_ragged_kernel(const TileJob *jobs, int n, const int *tables,
                                                                           const uint8_t *scratch)
{
    const TMF_CONST_AS TileJob *J = (const TMF_CONST_AS TileJob *)jobs;
    const uint32_t item = blockIdx.x;
    const int j = tile_find(n, item, [&](int i) { return J[i].v_item0; });
    tile_v_thread(J + j, item - J[j].v_item0, (int)threadIdx.x, (const TMF_CONST_AS int *)tables, scratch);
}

hipError_t launch_tiles_ragged(const TileJob *jobs, int64_t n, const int *tables, uint8_t *scratch, int64_t h_items,
                               int64_t v_items, hipStream_t st)
{
    if (n <= 0 || n > 0x7FFFFFFFll || h_items > kTileItemCap || v_items > kTileItemCap) return hipErrorInvalidValue;
    if (h_items > 0)
        hipLaunchKernelGGL(resample_h_ragged_kernel, dim3((unsigned)h_items), dim3(kTileSeg), 0, st, jobs, (int)n, tables, scratch);
    if (v_items > 0)
        hipLaunchKernelGGL(resample_v_paste_ragged_kernel, dim3((unsigned)v_items), dim3(kTileSeg), 0, st, jobs, (int)n, tables,
                           (const uint8_t *)scratch);
    return hipGetLastError();
}

static dim3 grid3(int w, int h, int64_t n) { return dim3((unsigned)((w + 255) / 256), (unsigned)h, (unsigned)n); }

// Image.resize((ow, oh), LANCZOS) of n images (ih x iw, in_stride bytes apart) into n outputs
// (row stride ldo, out_stride bytes apart), every pass one launch over a group of at most
// kResizeGroup images (the grid's z limit is 65535; the group also bounds the scratch).
// tables: device copy of [bounds_h | kk_h | bounds_v | kk_v] (ResamplePlan::pack),
// tmp: device scratch of resize_tmp_bytes(plan, n).
hipError_t launch_resize_lanczos_batch(const uint8_t *in, int64_t in_stride, int64_t n, const ResamplePlan &plan, const int *tables,
                                       uint8_t *tmp, uint8_t *out, int ldo, int64_t out_stride, hipStream_t st)
{
    const int ih = plan.ih, iw = plan.iw, oh = plan.oh, ow = plan.ow;
    const int *bh = tables, *kh = bh + plan.h.bounds.size(), *bv = kh + plan.h.kk.size(), *kv = bv + plan.v.bounds.size();
    const int64_t tstride = (int64_t)plan.tmp_bytes();
    for (int64_t i0 = 0; i0 < n; i0 += kResizeGroup) {
        const int64_t g = n - i0 < kResizeGroup ? n - i0 : kResizeGroup;
        const uint8_t *gin = in + i0 * in_stride;
        uint8_t *gout = out + i0 * out_stride;
        if (oh == ih && ow == iw) {  // Image.resize returns a copy
            hipLaunchKernelGGL(copy_rows_kernel, grid3(iw, ih, g), dim3(256), 0, st, gin, in_stride, iw, ih, gout, out_stride, ldo);
            continue;
        }
        const uint8_t *src = gin;
        int64_t sstride = in_stride;
        int sw = iw;
        if (plan.need_h) {  // the groups share the scratch: they run in stream order
            hipLaunchKernelGGL(resample_h_kernel, grid3(ow, plan.rows(), g), dim3(256), 0, st, gin, in_stride, iw, plan.y_first,
                               plan.rows(), ow, bh, kh, plan.h.ksize, tmp, tstride, ow);
            src = tmp;
            sstride = tstride;
            sw = ow;
        }
        if (plan.need_v)
            hipLaunchKernelGGL(resample_v_kernel, grid3(sw, oh, g), dim3(256), 0, st, src, sstride, sw, oh, bv, kv, plan.v.ksize,
                               gout, out_stride, ldo);
        else
            hipLaunchKernelGGL(copy_rows_kernel, grid3(sw, oh, g), dim3(256), 0, st, src, sstride, sw, oh, gout, out_stride, ldo);
    }
    return hipGetLastError();
}

size_t resize_tmp_bytes(const ResamplePlan &plan, int64_t n)
{
    return plan.tmp_bytes() * (size_t)(n < kResizeGroup ? n : kResizeGroup);
}

// one image: tmp is device scratch of plan.tmp_bytes()
hipError_t launch_resize_lanczos(const uint8_t *in, const ResamplePlan &plan, const int *tables, uint8_t *tmp, uint8_t *out,
                                 int ldo, hipStream_t st)
{
    return launch_resize_lanczos_batch(in, 0, 1, plan, tables, tmp, out, ldo, 0, st);
}

void ResamplePlan::build(int in_h, int in_w, int out_h, int out_w)
{
    ih = in_h;
    iw = in_w;
    oh = out_h;
    ow = out_w;
    need_h = ow != iw;
    need_v = oh != ih;
    h.build(iw, ow);
    v.build(ih, oh);
    y_first = v.bounds[0];
    y_last = v.bounds[(size_t)oh * 2 - 2] + v.bounds[(size_t)oh * 2 - 1];
    if (need_h)  // the vertical pass reads the horizontally resampled rows [y_first, y_last)
        for (int i = 0; i < oh; i++) v.bounds[(size_t)i * 2] -= y_first;
}

std::vector<int> ResamplePlan::pack() const
{
    std::vector<int> t;
    t.reserve(h.bounds.size() + h.kk.size() + v.bounds.size() + v.kk.size());
    t.insert(t.end(), h.bounds.begin(), h.bounds.end());
    t.insert(t.end(), h.kk.begin(), h.kk.end());
    t.insert(t.end(), v.bounds.begin(), v.bounds.end());
    t.insert(t.end(), v.kk.begin(), v.kk.end());
    return t;
}

}  // namespace tmf
