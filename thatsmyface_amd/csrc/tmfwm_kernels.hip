// HIP kernels of the watermark path for gfx950 (MI355X).
//
// Layout in HBM: frames are H x W x 3 u8, HWC-interleaved (PIL / numpy order), frame
// i at base + i * frame_stride.  The watermark tile is (H/b) x (W/b) u8, frame i's
// at wm + i * wm_stride (stride 0: one tile shared by every frame of a batch).  Extracted tiles are (H/b) x (W/b) u8 per frame.
//
// Work decomposition: a workgroup is ONE wave of 64 lanes that owns a
// strip of 64/L horizontally adjacent b x b blocks of one block row of one frame;
// L lanes cooperate on each block, lane q of a block group holding rows
// [q*R, q*R + R) (R = b / L) of the block's pixels, of A = D*V and of V.
// Transposes for the column passes of the DCT / IDCT go through a padded LDS tile.
// Nothing is written to HBM between the uint8 load and the uint8 store.
#include "tmfwm_blocks.h"
#include "tmfwm_passes.h"

namespace tmf {

extern template __global__ void embed_kernel<8, false>(EmbedArgs);  // tmfwm_embed8.hip
extern template __global__ void embed_kernel<8, true>(EmbedArgs);

// Extract's strip pass and list pass (extract_sigmas, extract_byte and their constants: tmfwm_passes.h)
template <int B, bool LIST = false>
__global__ __launch_bounds__(64, (B > 8 ? 2 : kExtract8Waves)) void extract_kernel(ExtractArgs a)  // waves per SIMD
{
    constexpr int L = Geo<B>::L, BPW = Geo<B>::BPW, LD = B + 1;
    __shared__ float lds[BPW * B * LD];
    const int lane = threadIdx.x & 63, g = lane / L, q = lane % L;
    float *tile = lds + g * B * LD;
    if constexpr (LIST) {
        // grid-stride over the list's segments: the blocks the strip pass left undecided
        const uint32_t per_frame = (uint32_t)a.nbh * (uint32_t)a.nbw, rows = (uint32_t)a.nframes * (uint32_t)a.nbh;
        for (uint32_t s = blockIdx.x; s < kListShards; s += gridDim.x) {
          const uint32_t n = a.slow_shards[s * kShardStride], base = shard_base(s, rows, (uint32_t)a.nbw);
          if (n != 0 && lane == 0) atomicAdd(a.slow_count, n);
          for (uint32_t t0 = 0; t0 < n; t0 += BPW) {
            StripPos pos;
            pos.valid = t0 + g < n;
            const uint32_t id = pos.valid ? a.slow_list[base + t0 + g] : 0u;
            pos.frame = id / per_frame;
            const uint32_t rem = id % per_frame;
            pos.bi = (int)(rem / (uint32_t)a.nbw);
            pos.bj = (int)(rem % (uint32_t)a.nbw);
            float sw, so;
            bool ok;
            extract_sigmas<B, kListPowerIters>(a, pos, tile, q, sw, so, ok);
            if (pos.valid && q == 0) {
                if (ok) a.out[pos.frame * a.tile_stride + (int64_t)pos.bi * a.nbw + pos.bj] = extract_byte(sw, so, a.alpha32);
                else a.fb_list[atomicAdd(a.fb_count, 1u)] = id;  // dgesdd route (extract_fixup_kernel)
            }
            __syncthreads();  // the LDS tiles are reused by the next listed blocks
          }
        }
    } else {
        const StripPos pos = strip_pos<B>(a.strips_per_row, a.nbw);
        float sw, so;
        bool ok;
        extract_sigmas<B, kPowerIters>(a, pos, tile, q, sw, so, ok);
        if (!pos.valid || q != 0) return;
        const uint32_t id = (uint32_t)(((int64_t)blockIdx.y * a.nbh + pos.bi) * a.nbw + pos.bj);
        if (!ok) {  // the enclosure did not decide f32(sigma_1): list pass, or the dgesdd route
            if (a.slow_list) {
                const uint32_t row = blockIdx.y * (uint32_t)a.nbh + (uint32_t)pos.bi, s = row % kListShards;
                a.slow_list[shard_base(s, (uint32_t)a.nframes * (uint32_t)a.nbh, (uint32_t)a.nbw) +
                            atomicAdd(a.slow_shards + s * kShardStride, 1u)] = id;
            }
            else a.fb_list[atomicAdd(a.fb_count, 1u)] = id;
            return;
        }
        a.out[pos.frame * a.tile_stride + (int64_t)pos.bi * a.nbw + pos.bj] = extract_byte(sw, so, a.alpha32);
    }
}

// ---------------------------------------------------------------------------
// Pixels outside the full-block grid only get the colour round trip (:166, :216).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void edge_roundtrip_kernel(EdgeArgs a)
{
    edge_roundtrip_pixel(a, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, blockIdx.y * a.frame_stride);
}

// ---------------------------------------------------------------------------
// Module-level helpers of the reference API (rgb_to_ycbcr :23, ycbcr_to_rgb :53,
// apply_dct_to_block :76, apply_idct_to_block :81) and the SVD stage on its own.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rgb_to_ycbcr_kernel(const uint8_t *__restrict__ rgb, int64_t npix, float *__restrict__ ycc)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const uint32_t r = rgb[3 * p], g = rgb[3 * p + 1], b = rgb[3 * p + 2];
    float cbs, crs;
    chroma(r, g, b, cbs, crs);
    ycc[3 * p] = luma(r, g, b);
    ycc[3 * p + 1] = cbs;
    ycc[3 * p + 2] = crs;
}

__global__ __launch_bounds__(256) void rgb_to_ycbcr_f32_kernel(const float *__restrict__ rgb, int64_t npix, float *__restrict__ ycc)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    colour_fwd_f32(rgb[3 * p], rgb[3 * p + 1], rgb[3 * p + 2], ycc[3 * p], ycc[3 * p + 1], ycc[3 * p + 2]);
}

template <typename T>
__global__ __launch_bounds__(256) void ycbcr_to_rgb_kernel(const T *__restrict__ ycc, int64_t npix, uint8_t *__restrict__ rgb)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    uint32_t R8, G8, B8;
    colour_inv_t<T>(ycc[3 * p], ycc[3 * p + 1], ycc[3 * p + 2], R8, G8, B8);
    rgb[3 * p] = (uint8_t)R8;
    rgb[3 * p + 1] = (uint8_t)G8;
    rgb[3 * p + 2] = (uint8_t)B8;
}

template <int B, bool INVERSE>
__global__ __launch_bounds__(64) void dct2d_blocks_kernel(float *blocks, int64_t nblocks)
{
    constexpr int L = Geo<B>::L, R = Geo<B>::R, BPW = Geo<B>::BPW, LD = B + 1;
    __shared__ float lds[BPW * B * LD];
    const int lane = threadIdx.x & 63, g = lane / L, q = lane % L;
    const int64_t blk = (int64_t)blockIdx.x * BPW + g;
    const bool valid = blk < nblocks;
    float x[R][B];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int c = 0; c < B; ++c) x[r][c] = valid && real_row<B>(q, r) ? blocks[blk * B * B + (q * R + r) * B + c] : 0.0f;
    dct2d_rows_layout<B, INVERSE>(x, lds + g * B * LD, q);
    if (valid)
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (real_row<B>(q, r))
#pragma unroll
                for (int c = 0; c < B; ++c) blocks[blk * B * B + (q * R + r) * B + c] = x[r][c];
}

template <int B>
__global__ __launch_bounds__(64) void svd_blocks_kernel(const float *__restrict__ D, int64_t nblocks, float *__restrict__ U,
                                                        float *__restrict__ S, float *__restrict__ Vt, int32_t *__restrict__ sweeps)
{
    constexpr int L = Geo<B>::L, R = Geo<B>::R, BPW = Geo<B>::BPW;
    constexpr int SD = (kScratchFloats<B, L> + 1) / 2;
    __shared__ double norms[BPW * SD];  // svd3's per-block LDS scratch
    const int lane = threadIdx.x & 63, g = lane / L, q = lane % L;
    const int64_t blk = (int64_t)blockIdx.x * BPW + g;
    const bool valid = blk < nblocks;
    float x[R][B];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int c = 0; c < B; ++c) x[r][c] = valid && real_row<B>(q, r) ? D[blk * B * B + (q * R + r) * B + c] : 0.0f;
    double A[R][B], V[R][B];
    int nsw = svd3<B, L>(x, A, V, q, NoStamp{}, norms + g * SD);
    double sig[B];
    float Uf[R][B], Vf[R][B];
#pragma unroll
    for (int k = 0; k < B; ++k) sig[k] = cdot_part<R, B>(A, k, k);
#pragma unroll
    for (int k = 0; k < B; ++k) {
        sig[k] = __builtin_sqrt(group_sum<L>(sig[k]));
        const double inv = 1.0 / sig[k];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            Uf[r][k] = sig[k] == 0.0 ? 0.0f : (float)(A[r][k] * inv);
            Vf[r][k] = (float)V[r][k];
        }
    }
    bool zero = true;
#pragma unroll
    for (int k = 0; k < B; ++k) zero = zero && (sig[k] == 0.0);
    if (zero) {
        nsw = 0;  // oracle: D == 0 returns before any sweep
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int k = 0; k < B; ++k) Uf[r][k] = Vf[r][k] = (q * R + r == k) ? 1.0f : 0.0f;
    }
#pragma unroll
    for (int round = 0; round < B; ++round)
#pragma unroll
        for (int k = round & 1; k + 1 < B; k += 2) {
            const bool sw = sig[k] < sig[k + 1];
            const double s0 = sig[k], s1 = sig[k + 1];
            sig[k] = sw ? s1 : s0;
            sig[k + 1] = sw ? s0 : s1;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float u0 = Uf[r][k], u1 = Uf[r][k + 1], v0 = Vf[r][k], v1 = Vf[r][k + 1];
                Uf[r][k] = sw ? u1 : u0;
                Uf[r][k + 1] = sw ? u0 : u1;
                Vf[r][k] = sw ? v1 : v0;
                Vf[r][k + 1] = sw ? v0 : v1;
            }
        }
    if (!valid) return;
#pragma unroll
    for (int r = 0; r < R; ++r)
        if (real_row<B>(q, r))
#pragma unroll
            for (int k = 0; k < B; ++k) {
                U[blk * B * B + (q * R + r) * B + k] = Uf[r][k];
                Vt[blk * B * B + k * B + q * R + r] = Vf[r][k];
            }
    if (q == 0) {
#pragma unroll
        for (int k = 0; k < B; ++k) S[blk * B + k] = (float)sig[k];
        if (sweeps) sweeps[blk] = nsw;
    }
}

// ---------------------------------------------------------------------------
// Synthetic frames for the benchmark, generated in HBM:
// byte = splitmix64(seed ^ (frame << 40) ^ idx) & 0xFF.
// ---------------------------------------------------------------------------
TMF_DEVI uint64_t splitmix64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ULL;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    return x ^ (x >> 31);
}

__global__ __launch_bounds__(256) void synth_kernel(uint64_t seed, int64_t frame0, int64_t frame_bytes, uint8_t *out)
{
    const int64_t f = blockIdx.y;
    const uint64_t fs = seed ^ ((uint64_t)(frame0 + f) << 40);
    uint8_t *o = out + f * frame_bytes;
    for (int64_t i4 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i4 < frame_bytes; i4 += (int64_t)gridDim.x * blockDim.x * 4) {
        if (i4 + 4 <= frame_bytes && ((reinterpret_cast<uintptr_t>(o + i4) & 3) == 0)) {
            uint32_t w = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) w |= (uint32_t)(splitmix64(fs ^ (uint64_t)(i4 + k)) & 0xFF) << (8 * k);
            *reinterpret_cast<uint32_t *>(o + i4) = w;
        } else {
            for (int64_t i = i4; i < i4 + 4 && i < frame_bytes; ++i) o[i] = (uint8_t)(splitmix64(fs ^ (uint64_t)i) & 0xFF);
        }
    }
}

// ---------------------------------------------------------------------------
// Launchers (host side of this TU)
// ---------------------------------------------------------------------------
bool embed_defers(int block)
{
    return block_value(block, false, [](auto b) { return kDeferMax<b()> > 0; });
}

bool embed_key_fused(int block)
{
    return block_value(block, false, [](auto b) { return kEmbedKeyFused<b()>; });
}

// the key variants of the strip and list passes, one TU per block size (tmfwm_embed_key.hip)
hipError_t launch_embed_key_strips(const EmbedArgs &a, hipStream_t st)
{
    return for_block(a.block, [&](auto b) { return embed_key_strips_b<b()>(a, st); });
}

hipError_t launch_embed(const EmbedArgs &a, hipStream_t st)
{
    if (a.nbh > 0 && a.nbw > 0) {
        // the list pass takes the blocks the first pass left unfinished (ids relative to a.src)
        const hipError_t e = a.key_out ? launch_embed_key_strips(a, st) : for_block(a.block, [&](auto b) {
            constexpr int B = b();
            void (*list)(EmbedArgs) = nullptr;
            if constexpr (kDeferMax<B> > 0) list = embed_kernel<B, true>;
            return launch_strips(a, Geo<B>::BPW, embed_kernel<B, false>, list, st);
        });
        if (e != hipSuccess) return e;
    }
    return launch_edges(a.src, a.dst, a.nframes, a.H, a.W, a.frame_stride, a.block, st);
}

hipError_t launch_edges(const uint8_t *src, uint8_t *dst, int64_t nframes, int H, int W, int64_t frame_stride, int block, hipStream_t st)
{
    EdgeArgs e;
    e.src = src;
    e.dst = dst;
    e.H = H;
    e.W = W;
    e.frame_stride = frame_stride;
    e.core_h = (H / block) * block;
    e.core_w = (W / block) * block;
    e.edge_w = W - e.core_w;
    const int64_t n = (int64_t)e.core_h * e.edge_w + (int64_t)(H - e.core_h) * W;
    if (n == 0) return hipSuccess;
    return for_frame_slices(nframes, [&](int64_t f0, int64_t nf) {
        EdgeArgs c = e;
        c.src = src + f0 * frame_stride;
        c.dst = dst + f0 * frame_stride;
        hipLaunchKernelGGL(edge_roundtrip_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)nf), dim3(256), 0, st, c);
    });
}

hipError_t launch_extract(const ExtractArgs &a, hipStream_t st)
{
    if (a.nbh == 0 || a.nbw == 0) return hipSuccess;
    // the list pass takes the undecided blocks (ids relative to a.wsrc / a.osrc)
    return for_block(a.block, [&](auto b) {
        return launch_strips(a, Geo<b()>::BPW, extract_kernel<b(), false>, extract_kernel<b(), true>, st);
    });
}

hipError_t launch_rgb_to_ycbcr(const uint8_t *rgb, int64_t npix, float *ycc, hipStream_t st)
{
    if (npix == 0) return hipSuccess;
    hipLaunchKernelGGL(rgb_to_ycbcr_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, st, rgb, npix, ycc);
    return hipGetLastError();
}

hipError_t launch_rgb_to_ycbcr_f32(const float *rgb, int64_t npix, float *ycc, hipStream_t st)
{
    if (npix == 0) return hipSuccess;
    hipLaunchKernelGGL(rgb_to_ycbcr_f32_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, st, rgb, npix, ycc);
    return hipGetLastError();
}

hipError_t launch_ycbcr_to_rgb(const void *ycc, int dtype, int64_t npix, uint8_t *rgb, hipStream_t st)
{
    if (npix == 0) return hipSuccess;
    const dim3 grid((unsigned)((npix + 255) / 256));
    switch (dtype) {
    case TMFWM_DT_F16:
        hipLaunchKernelGGL(ycbcr_to_rgb_kernel<_Float16>, grid, dim3(256), 0, st, static_cast<const _Float16 *>(ycc), npix, rgb);
        break;
    case TMFWM_DT_F32:
        hipLaunchKernelGGL(ycbcr_to_rgb_kernel<float>, grid, dim3(256), 0, st, static_cast<const float *>(ycc), npix, rgb);
        break;
    case TMFWM_DT_F64:
        hipLaunchKernelGGL(ycbcr_to_rgb_kernel<double>, grid, dim3(256), 0, st, static_cast<const double *>(ycc), npix, rgb);
        break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_dct2d_blocks(float *blocks, int64_t nb, int block, int inverse, hipStream_t st)
{
    if (nb == 0) return hipSuccess;
    return for_block(block, [&](auto b) {
        constexpr int B = b();
        const unsigned grid = (unsigned)((nb + Geo<B>::BPW - 1) / Geo<B>::BPW);
        if (inverse) hipLaunchKernelGGL((dct2d_blocks_kernel<B, true>), dim3(grid), dim3(64), 0, st, blocks, nb);
        else hipLaunchKernelGGL((dct2d_blocks_kernel<B, false>), dim3(grid), dim3(64), 0, st, blocks, nb);
        return hipGetLastError();
    });
}

hipError_t launch_svd_blocks(const float *D, int64_t nb, int block, float *U, float *S, float *Vt, int32_t *sweeps, hipStream_t st)
{
    if (nb == 0) return hipSuccess;
    return for_block(block, [&](auto b) {
        constexpr int B = b();
        const unsigned grid = (unsigned)((nb + Geo<B>::BPW - 1) / Geo<B>::BPW);
        hipLaunchKernelGGL(svd_blocks_kernel<B>, dim3(grid), dim3(64), 0, st, D, nb, U, S, Vt, sweeps);
        return hipGetLastError();
    });
}

#ifdef TMF_STAMPS
extern "C" int tmfwm_debug_stamps(unsigned long long *out, int reset)
{
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps), sizeof(unsigned long long) * 16) != hipSuccess) return -5;
    if (reset) {
        unsigned long long z[16] = {};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), z, sizeof z) != hipSuccess) return -5;
    }
    return 0;
}
#endif

hipError_t launch_synth(uint64_t seed, int64_t frame0, int64_t nframes, int64_t frame_bytes, uint8_t *out, hipStream_t st)
{
    if (nframes == 0 || frame_bytes == 0) return hipSuccess;
    const int64_t per = (frame_bytes + 1023) / 1024;
    const unsigned gx = (unsigned)(per < 4096 ? per : 4096);
    return for_frame_slices(nframes, [&](int64_t f0, int64_t nf) {
        hipLaunchKernelGGL(synth_kernel, dim3(gx, (unsigned)nf), dim3(256), 0, st, seed, frame0 + f0, frame_bytes, out + f0 * frame_bytes);
    });
}

}  // namespace tmf
