// Key variants of the single-size embed passes (tmfwm_blocks.h: embed_key_kernel;
// tmfwm_embed_key.h) for one block size, TMF_B: the strip pass and b = 8's list
// pass.  The Makefile compiles this file once per size (tmfwm_embed_key<b>.o), b = 8 under the
// max-ILP scheduler as its plain sibling embed_kernel<8> (tmfwm_embed8.hip).  The ragged strip
// pass and the dgesdd-route passes sit beside the plain ones (tmfwm_ragged_strip.hip,
// tmfwm_fixup.hip, tmfwm_ragged_fixup.hip).
#include "tmfwm_blocks.h"

#ifndef TMF_B
#error "TMF_B: the block size of this translation unit"
#endif

namespace tmf {

template <int B>
hipError_t embed_key_strips_b(const EmbedArgs &a, hipStream_t st)
{
    // the list pass takes the blocks the first pass left unfinished, their key entries with them
    void (*list)(EmbedArgs) = nullptr;
    if constexpr (kDeferMax<B> > 0) list = embed_key_kernel<B, true>;
    return launch_strips(a, Geo<B>::BPW, embed_key_kernel<B, false>, list, st);
}

template hipError_t embed_key_strips_b<TMF_B>(const EmbedArgs &, hipStream_t);

}  // namespace tmf
