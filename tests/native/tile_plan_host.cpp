// TEST-ONLY: the plan of a ragged tile preparation (thatsmyface_amd/csrc/tmfwm_tile_plan.h) built
// on the host CPU, and both passes walked exactly as the two grids run them -- work item ->
// prefix search -> the per-thread body the kernels call -- so that tests/test_tiles_ragged.py can
// check the index arithmetic against the oracle without a GPU.  Built by that test; never shipped.
#include <stdint.h>

#include <vector>

#include "../../thatsmyface_amd/csrc/tmfwm_tile_plan.h"

extern "C" {

int tp_segment(void) { return tmf::kTileSeg; }
int tp_job_bytes(void) { return (int)sizeof(tmf::TileJob); }
long long tp_default_cap(void) { return tmf::kTileScratchCap; }

// sizes: n x (wm_height, wm_width, tile_height, tile_width); job i reads wm + wm_off[i] and writes
// out + tile_off[i].  info: axes built, groups, scratch bytes, launches.  Returns -1, or the job
// the plan refuses.
long long tp_run(const int32_t *sizes, long long n, const uint8_t *wm, const long long *wm_off, uint8_t *out,
                 const long long *tile_off, int preserve_ratio, long long scratch_cap, long long *info)
{
    std::vector<tmf::TileJobIn> in((size_t)n);
    for (long long i = 0; i < n; ++i)
        in[(size_t)i] = {wm + wm_off[i], out + tile_off[i], sizes[4 * i], sizes[4 * i + 1], sizes[4 * i + 2], sizes[4 * i + 3]};
    tmf::TilePlan plan;
    const char *why = "";
    const long long bad = plan.build(in.data(), n, preserve_ratio != 0, scratch_cap, &why);
    if (bad >= 0) return bad;
    // one scratch for all groups, as on the device; never zero-filled there either
    std::vector<uint8_t> scratch((size_t)plan.scratch + 1, 0xCD);
    const int *tables = plan.tables.data();
    long long launches = 0;
    for (const tmf::TileGroup &g : plan.groups) {
        const tmf::TileJob *jobs = plan.jobs.data() + g.first;
        if (g.scratch > plan.scratch) return -2;
        if (g.h_items > 0) {
            ++launches;
            for (int64_t item = 0; item < g.h_items; ++item) {
                const int j = tmf::tile_find((int)g.n, (uint32_t)item, [&](int i) { return jobs[i].h_item0; });
                if (!jobs[j].need_h || jobs[j].scratch + (int64_t)jobs[j].rows * jobs[j].rw > g.scratch) return -3;
                for (int lane = 0; lane < tmf::kTileSeg; ++lane)
                    tmf::tile_h_thread(jobs + j, (uint32_t)item - jobs[j].h_item0, lane, tables, scratch.data());
            }
        }
        ++launches;
        for (int64_t item = 0; item < g.v_items; ++item) {
            const int j = tmf::tile_find((int)g.n, (uint32_t)item, [&](int i) { return jobs[i].v_item0; });
            for (int lane = 0; lane < tmf::kTileSeg; ++lane)
                tmf::tile_v_thread(jobs + j, (uint32_t)item - jobs[j].v_item0, lane, tables, (const uint8_t *)scratch.data());
        }
    }
    info[0] = plan.axes;
    info[1] = (long long)plan.groups.size();
    info[2] = plan.scratch;
    info[3] = launches;
    return -1;
}

}  // extern "C"
