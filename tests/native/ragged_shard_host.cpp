// Host build of the ragged list pass's segment layout (tmfwm_ragged.h: ragged_plan_shards,
// ragged_seg_base, ragged_shards_full) for tests/test_ragged_rank1.py.  Frames of nbh[i] x nbw[i]
// blocks are cut into chunks as the C ABI cuts them on TMFWM_ROUTE_RANK1 (at most `cap` blocks, a
// frame that alone has more being a chunk of its own, and at most kListShards frames with blocks);
// in every chunk the segments of all (frame, shard) pairs, in table order, must lie back to back
// from 0 to the chunk's blocks, each exactly as long as the rows dealt to it.
#include <vector>

#include "../../thatsmyface_amd/csrc/tmfwm_ragged.h"

namespace {
struct Fr {
    int32_t nbh, nbw;
    uint32_t block0;
};

int check_chunk(const std::vector<Fr> &f)
{
    using namespace tmf;
    std::vector<RaggedShards> sh(f.size());
    const uint32_t used = ragged_plan_shards(f.data(), (int64_t)f.size(), sh.data());
    if (used > kListShards) return 1;
    uint32_t expect = 0, next_shard = 0;
    for (size_t i = 0; i < f.size(); ++i) {
        const uint32_t nbh = (uint32_t)f[i].nbh, nbw = (uint32_t)f[i].nbw, n = sh[i].n;
        if (sh[i].sh0 != next_shard) return 2;  // contiguous ranges in table order
        if (nbh == 0 || nbw == 0) {
            if (n != 0) return 3;
            continue;
        }
        if (n < 1 || n > nbh) return 4;
        if (f[i].block0 != expect) return 5;
        for (uint32_t k = 0; k < n; ++k) {
            if (ragged_seg_base(f[i].block0, nbh, nbw, n, k) != expect) return 6;
            uint32_t rows = 0;
            for (uint32_t bi = k; bi < nbh; bi += n) ++rows;  // the rows with bi % n == k
            expect += rows * nbw;
        }
        if (ragged_seg_base(f[i].block0, nbh, nbw, n, n) != expect) return 7;
        if (expect != f[i].block0 + nbh * nbw) return 8;
        next_shard += n;
    }
    return next_shard == used ? 0 : 9;
}
}  // namespace

// 0, or the first failed check * 1000 + the chunk's number; *n_chunks: how many chunks the frames made
extern "C" int ragged_shard_check(const int32_t *nbh, const int32_t *nbw, int64_t n, int64_t cap, int64_t *n_chunks)
{
    std::vector<Fr> chunk;
    int64_t blocks = 0, with_blocks = 0, chunks = 0;
    auto close = [&]() -> int {
        const int rc = chunk.empty() ? 0 : check_chunk(chunk);
        chunks += !chunk.empty();
        chunk.clear();
        blocks = with_blocks = 0;
        return rc ? rc * 1000 + (int)chunks : 0;
    };
    for (int64_t i = 0; i < n; ++i) {
        const int64_t b = (int64_t)nbh[i] * nbw[i];
        if (!chunk.empty() && (blocks + b > cap || (b > 0 && tmf::ragged_shards_full(with_blocks))))
            if (int rc = close()) return rc;
        chunk.push_back({nbh[i], nbw[i], (uint32_t)blocks});
        blocks += b;
        with_blocks += b > 0;
    }
    if (int rc = close()) return rc;
    *n_chunks = chunks;
    return 0;
}

extern "C" uint32_t ragged_shard_count() { return tmf::kListShards; }
