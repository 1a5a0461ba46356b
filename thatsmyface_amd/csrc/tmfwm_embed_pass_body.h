// The body of the single-size embed passes: the one text of embed_kernel<B, LIST> and
// embed_key_kernel<B, LIST> (tmfwm_blocks.h), which differ in embed_blocks' KEY alone.  No include
// guard and no namespace: each kernel includes it inside its own braces.  A fragment and not a
// device function: with both kernels calling one function for it, embed_kernel<8> compiled to 256
// VGPRs and 56 bytes of scratch instead of 255 and none; included, each kernel compiles to the
// instructions it had with the body written out (profiles/one_body/).
//
// Expected in scope: B, LIST, a (the kernel's EmbedArgs), and constexpr bool KEY.
    constexpr int L = Geo<B>::L, BPW = Geo<B>::BPW, TS = kEmbedTS<B>;
    // the transpose tiles (also svd3's scratch during the SVD), then the source bytes / the
    // upper-end tiles, in one array (the reconstruction picks a tile by an offset)
    __shared__ __attribute__((aligned(16))) float lds_all[BPW * TS + kHiPad<B> + kLds2Floats<B>];
    float *lds = lds_all, *lds2 = lds_all + BPW * TS + kHiPad<B>;
    if constexpr (LIST) {
        // grid-stride over the slow list's segments (their lengths are known on the device only)
        const uint32_t per_frame = (uint32_t)a.nbh * (uint32_t)a.nbw, rows = (uint32_t)a.nframes * (uint32_t)a.nbh;
        const int g = (threadIdx.x & 63) / L;
        for (uint32_t s = blockIdx.x; s < kListShards; s += gridDim.x) {
            const uint32_t n = a.slow_shards[s * kShardStride], base = shard_base(s, rows, (uint32_t)a.nbw);
            if (n != 0 && (threadIdx.x & 63) == 0) atomicAdd(a.slow_count, n);
            for (uint32_t t0 = 0; t0 < n; t0 += BPW) {
                StripPos pos;
                pos.valid = t0 + g < n;
                const uint32_t id = pos.valid ? a.slow_list[base + t0 + g] : 0u;
                pos.frame = id / per_frame;
                const uint32_t rem = id % per_frame;
                pos.bi = (int)(rem / (uint32_t)a.nbw);
                pos.bj = (int)(rem % (uint32_t)a.nbw);
                embed_blocks<B, true, KEY>(a, pos, id, lds, lds2);
                __syncthreads();  // the LDS tiles are reused by the next listed blocks
            }
        }
    } else {
        const StripPos pos = strip_pos<B>(a.strips_per_row, a.nbw);
        const uint32_t id = (uint32_t)(((int64_t)blockIdx.y * a.nbh + pos.bi) * a.nbw + pos.bj);
        embed_blocks<B, false, KEY>(a, pos, id, lds, lds2);
    }
