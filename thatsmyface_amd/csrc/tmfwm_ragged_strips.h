// What every ragged strip kernel starts with (tmfwm_ragged_strip.hip, tmfwm_ragged_pre.hip):
// the wave's frame in the table's wave prefix and its strip of that frame.
#pragma once
#include "tmfwm_blocks.h"
#include "tmfwm_ragged.h"

namespace tmf {

// this wave's strip of frame f (frame index 0 of the one-frame view) and its first block's id
template <int B>
TMF_DEVI StripPos ragged_strip_pos(RaggedFrameK *f, uint32_t &id)
{
    const uint32_t w = blockIdx.x - f->wave0, spr = (uint32_t)f->strips_per_row;
    StripPos p;
    p.frame = 0;
    p.bi = (int)(w / spr);
    p.bj = (int)(w % spr) * Geo<B>::BPW + (int)(threadIdx.x & 63) / Geo<B>::L;
    p.valid = p.bj < f->nbw;
    id = f->block0 + (uint32_t)p.bi * (uint32_t)f->nbw + (uint32_t)p.bj;
    return p;
}

TMF_DEVI RaggedFrameK *ragged_wave_frame(const RaggedArgs &r)
{
    RaggedFrameK *tab = ragged_const(r.frames);
    return tab + ragged_find(r.nframes, blockIdx.x, [&](int i) { return tab[i].wave0; });
}

}  // namespace tmf
