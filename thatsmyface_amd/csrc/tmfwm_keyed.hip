// Keyed extraction: the strip pass and the list pass over ONE image per frame (tmfwm_keyed.h,
// DESIGN.md 5).  The work decomposition is extract_kernel's (tmfwm_kernels.hip): a workgroup
// is one wave that owns a strip of 64 / L adjacent blocks of one block row, L lanes per block.
//
//   sigma1_map_kernel      key[frame][bi][bj] = f32(sigma_1) of the block
//   extract_keyed_kernel   out[frame][bi][bj] = extract_byte(sigma_1 of the block, key entry, alpha)
//   sigma1_map_px4_kernel, extract_keyed_px4_kernel   the same on frames of 4-byte pixels (R G B pad)
//
// A block whose enclosure does not decide f32(sigma_1) goes to the list pass (kListPowerIters)
// and from there to the dgesdd route (tmfwm_keyed_fixup.hip), as in the pair path.
#include "tmfwm_keyed.h"

namespace tmf {

// (kKeyedWaves and keyed_sigma, the strip body of one image: tmfwm_keyed.h)
template <int B, bool LIST, bool MAP, int PX = 3>
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
                keyed_sigma<B, kListPowerIters, PX>(a, pos, tile, q, s, ok);
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
        keyed_sigma<B, kPowerIters, PX>(a, pos, tile, q, s, ok);
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

// The same passes over frames of 4-byte pixels (R G B pad), read where they lie: kernels of their
// own, so that the 3-byte kernels above keep their names and their code.
template <int B, bool LIST = false>
__global__ __launch_bounds__(64, kKeyedWaves<B>) void sigma1_map_px4_kernel(KeyedArgs a)
{
    keyed_pass<B, LIST, true, 4>(a);
}

template <int B, bool LIST = false>
__global__ __launch_bounds__(64, kKeyedWaves<B>) void extract_keyed_px4_kernel(KeyedArgs a)
{
    keyed_pass<B, LIST, false, 4>(a);
}

// the strip pass, then the list pass over the whole chunk (ids relative to a.src); px: the
// frames' bytes per pixel (3 or 4: the callers have checked it)
template <bool MAP>
static hipError_t launch_keyed(const KeyedArgs &a, hipStream_t st, int px)
{
    if (a.nbh == 0 || a.nbw == 0) return hipSuccess;
    if (px != 3 && px != 4) return hipErrorInvalidValue;
    return for_block(a.block, [&](auto b) {
        constexpr int B = b();
        if (px == 4) {
            if constexpr (MAP) return launch_strips(a, Geo<B>::BPW, sigma1_map_px4_kernel<B, false>, sigma1_map_px4_kernel<B, true>, st);
            else return launch_strips(a, Geo<B>::BPW, extract_keyed_px4_kernel<B, false>, extract_keyed_px4_kernel<B, true>, st);
        }
        if constexpr (MAP) return launch_strips(a, Geo<B>::BPW, sigma1_map_kernel<B, false>, sigma1_map_kernel<B, true>, st);
        else return launch_strips(a, Geo<B>::BPW, extract_keyed_kernel<B, false>, extract_keyed_kernel<B, true>, st);
    });
}

hipError_t launch_sigma1_map(const KeyedArgs &a, hipStream_t st, int px) { return launch_keyed<true>(a, st, px); }
hipError_t launch_extract_keyed(const KeyedArgs &a, hipStream_t st, int px) { return launch_keyed<false>(a, st, px); }

// the dgesdd-route passes, one TU per block size (tmfwm_keyed_fixup.hip)
hipError_t launch_sigma1_fixup(const KeyedArgs &a, const uint32_t *list, const uint32_t *count, int64_t max_entries, hipStream_t st,
                               int px)
{
    if (px != 3 && px != 4) return hipErrorInvalidValue;
    return for_block(a.block, [&](auto b) { return sigma1_fixup_b<b()>(a, list, count, max_entries, st, px); });
}

hipError_t launch_extract_keyed_fixup(const KeyedArgs &a, const uint32_t *list, const uint32_t *count, int64_t max_entries,
                                      hipStream_t st, int px)
{
    if (px != 3 && px != 4) return hipErrorInvalidValue;
    return for_block(a.block, [&](auto b) { return extract_keyed_fixup_b<b()>(a, list, count, max_entries, st, px); });
}

}  // namespace tmf
