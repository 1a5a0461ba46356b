// Keyed extraction: the strip pass and the list pass over ONE image per frame (tmfwm_keyed.h,
// DESIGN.md 5).  The work decomposition is extract_kernel's (tmfwm_kernels.hip): a workgroup
// is one wave that owns a strip of 64 / L adjacent blocks of one block row, L lanes per block.
//
//   sigma1_map_kernel      key[frame][bi][bj] = f32(sigma_1) of the block
//   extract_keyed_kernel   out[frame][bi][bj] = extract_byte(sigma_1 of the block, key entry, alpha)
//
// A block whose enclosure does not decide f32(sigma_1) goes to the list pass (kListPowerIters)
// and from there to the dgesdd route (tmfwm_keyed_fixup.hip), as in the pair path.
#include "tmfwm_keyed.h"

namespace tmf {

// waves per SIMD the register allocation must allow: one image's rows and one power iteration
// live at a time, so the pair kernels' bounds hold with room to spare
template <int B>
constexpr int kKeyedWaves = B > 8 ? 2 : kExtract8Waves;

// sigma_1 of this wave's blocks of the one image (pos per lane), certified or not (ok)
template <int B, int ITERS>
TMF_DEVI void keyed_sigma(const KeyedArgs &a, const StripPos &pos, float *tile, int q, float &s, bool &ok)
{
    constexpr int R = Geo<B>::R, L = Geo<B>::L;
    uint32_t w[R][Geo<B>::NW];
    float x[1][R][B], s1[1];
    bool k[1];
    load_block_rows<B>(a.src + pos.frame * a.frame_stride, a.W, pos, q, a.aligned, w);
    dct_rows_of<B>(w, q, tile, x[0]);
    sigma1_certified<B, L, ITERS, 1>(x, s1, k);
    s = s1[0];
    ok = k[0];
}

template <int B, bool LIST, bool MAP>
TMF_DEVI void keyed_pass(const KeyedArgs &a)
{
    constexpr int L = Geo<B>::L, BPW = Geo<B>::BPW, LD = B + 1;
    __shared__ float lds[BPW * B * LD];
    const int lane = threadIdx.x & 63, g = lane / L, q = lane % L;
    float *tile = lds + g * B * LD;
    if constexpr (LIST) {
        // grid-stride over the list's segments: the blocks the strip pass left undecided
        const uint32_t per_frame = (uint32_t)a.nbh * (uint32_t)a.nbw, rows = (uint32_t)a.nframes * (uint32_t)a.nbh;
        for (uint32_t sh = blockIdx.x; sh < kListShards; sh += gridDim.x) {
            const uint32_t n = a.slow_shards[sh * kShardStride], base = shard_base(sh, rows, (uint32_t)a.nbw);
            if (n != 0 && lane == 0) atomicAdd(a.slow_count, n);
            for (uint32_t t0 = 0; t0 < n; t0 += BPW) {
                StripPos pos;
                pos.valid = t0 + g < n;
                const uint32_t id = pos.valid ? a.slow_list[base + t0 + g] : 0u;
                pos.frame = id / per_frame;
                const uint32_t rem = id % per_frame;
                pos.bi = (int)(rem / (uint32_t)a.nbw);
                pos.bj = (int)(rem % (uint32_t)a.nbw);
                float s;
                bool ok;
                keyed_sigma<B, kListPowerIters>(a, pos, tile, q, s, ok);
                if (pos.valid && q == 0) {
                    if (ok) keyed_store<MAP>(a, pos.frame, pos.bi, pos.bj, s);
                    else a.fb_list[atomicAdd(a.fb_count, 1u)] = id;  // dgesdd route
                }
                __syncthreads();  // the LDS tiles are reused by the next listed blocks
            }
        }
    } else {
        const StripPos pos = strip_pos<B>(a.strips_per_row, a.nbw);
        float s;
        bool ok;
        keyed_sigma<B, kPowerIters>(a, pos, tile, q, s, ok);
        if (!pos.valid || q != 0) return;
        if (!ok) {  // the enclosure did not decide f32(sigma_1): list pass, or the dgesdd route
            const uint32_t id = (uint32_t)(((int64_t)blockIdx.y * a.nbh + pos.bi) * a.nbw + pos.bj);
            if (a.slow_list) {
                const uint32_t row = blockIdx.y * (uint32_t)a.nbh + (uint32_t)pos.bi, sh = row % kListShards;
                a.slow_list[shard_base(sh, (uint32_t)a.nframes * (uint32_t)a.nbh, (uint32_t)a.nbw) +
                            atomicAdd(a.slow_shards + sh * kShardStride, 1u)] = id;
            }
            else a.fb_list[atomicAdd(a.fb_count, 1u)] = id;
            return;
        }
        keyed_store<MAP>(a, pos.frame, pos.bi, pos.bj, s);
    }
}

template <int B, bool LIST = false>
__global__ __launch_bounds__(64, kKeyedWaves<B>) void sigma1_map_kernel(KeyedArgs a)
{
    keyed_pass<B, LIST, true>(a);
}

template <int B, bool LIST = false>
__global__ __launch_bounds__(64, kKeyedWaves<B>) void extract_keyed_kernel(KeyedArgs a)
{
    keyed_pass<B, LIST, false>(a);
}

// the strip pass in launches of at most 65535 frames (the grid's y limit; the frame pointers
// move with each launch), then the list pass over the whole chunk (ids relative to a.src)
template <int B, bool MAP>
static hipError_t launch_keyed_b(KeyedArgs a, hipStream_t st)
{
    a.strips_per_row = (a.nbw + Geo<B>::BPW - 1) / Geo<B>::BPW;
    const int64_t gx = (int64_t)a.strips_per_row * a.nbh;
    for (int64_t f0 = 0; f0 < a.nframes; f0 += 65535) {
        KeyedArgs c = a;
        const int64_t nf = a.nframes - f0 < 65535 ? a.nframes - f0 : 65535;
        c.src = a.src + f0 * a.frame_stride;
        if constexpr (MAP) {
            c.key_out = a.key_out + f0 * a.key_stride;
            hipLaunchKernelGGL((sigma1_map_kernel<B, false>), dim3((unsigned)gx, (unsigned)nf), dim3(64), 0, st, c);
        } else {
            c.key = a.key + f0 * a.key_stride;
            c.out = a.out + f0 * a.tile_stride;
            hipLaunchKernelGGL((extract_keyed_kernel<B, false>), dim3((unsigned)gx, (unsigned)nf), dim3(64), 0, st, c);
        }
    }
    if (a.slow_list) {
        const int64_t rows = a.nframes * a.nbh;  // segments past the rows stay empty
        const unsigned grid = (unsigned)(rows < (int64_t)kListShards ? rows : (int64_t)kListShards);
        if constexpr (MAP) hipLaunchKernelGGL((sigma1_map_kernel<B, true>), dim3(grid), dim3(64), 0, st, a);
        else hipLaunchKernelGGL((extract_keyed_kernel<B, true>), dim3(grid), dim3(64), 0, st, a);
    }
    return hipGetLastError();
}

template <bool MAP>
static hipError_t launch_keyed(const KeyedArgs &a, hipStream_t st)
{
    if (a.nbh == 0 || a.nbw == 0) return hipSuccess;
    switch (a.block) {
    case 4: return launch_keyed_b<4, MAP>(a, st);
    case 6: return launch_keyed_b<6, MAP>(a, st);
    case 8: return launch_keyed_b<8, MAP>(a, st);
    case 10: return launch_keyed_b<10, MAP>(a, st);
    case 12: return launch_keyed_b<12, MAP>(a, st);
    case 14: return launch_keyed_b<14, MAP>(a, st);
    case 16: return launch_keyed_b<16, MAP>(a, st);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_sigma1_map(const KeyedArgs &a, hipStream_t st) { return launch_keyed<true>(a, st); }
hipError_t launch_extract_keyed(const KeyedArgs &a, hipStream_t st) { return launch_keyed<false>(a, st); }

// the dgesdd-route passes, one TU per block size (tmfwm_keyed_fixup.hip)
#define TMF_KEYED_FIXUP_DECL(B)                                                                                      \
    hipError_t launch_sigma1_fixup_##B(const KeyedArgs &, const uint32_t *, const uint32_t *, int64_t, hipStream_t); \
    hipError_t launch_extract_keyed_fixup_##B(const KeyedArgs &, const uint32_t *, const uint32_t *, int64_t, hipStream_t);
TMF_KEYED_FIXUP_DECL(4)
TMF_KEYED_FIXUP_DECL(6)
TMF_KEYED_FIXUP_DECL(8)
TMF_KEYED_FIXUP_DECL(10)
TMF_KEYED_FIXUP_DECL(12)
TMF_KEYED_FIXUP_DECL(14)
TMF_KEYED_FIXUP_DECL(16)

hipError_t launch_sigma1_fixup(const KeyedArgs &a, const uint32_t *list, const uint32_t *count, int64_t max_entries, hipStream_t st)
{
    switch (a.block) {
    case 4: return launch_sigma1_fixup_4(a, list, count, max_entries, st);
    case 6: return launch_sigma1_fixup_6(a, list, count, max_entries, st);
    case 8: return launch_sigma1_fixup_8(a, list, count, max_entries, st);
    case 10: return launch_sigma1_fixup_10(a, list, count, max_entries, st);
    case 12: return launch_sigma1_fixup_12(a, list, count, max_entries, st);
    case 14: return launch_sigma1_fixup_14(a, list, count, max_entries, st);
    case 16: return launch_sigma1_fixup_16(a, list, count, max_entries, st);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_extract_keyed_fixup(const KeyedArgs &a, const uint32_t *list, const uint32_t *count, int64_t max_entries,
                                      hipStream_t st)
{
    switch (a.block) {
    case 4: return launch_extract_keyed_fixup_4(a, list, count, max_entries, st);
    case 6: return launch_extract_keyed_fixup_6(a, list, count, max_entries, st);
    case 8: return launch_extract_keyed_fixup_8(a, list, count, max_entries, st);
    case 10: return launch_extract_keyed_fixup_10(a, list, count, max_entries, st);
    case 12: return launch_extract_keyed_fixup_12(a, list, count, max_entries, st);
    case 14: return launch_extract_keyed_fixup_14(a, list, count, max_entries, st);
    case 16: return launch_extract_keyed_fixup_16(a, list, count, max_entries, st);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace tmf
