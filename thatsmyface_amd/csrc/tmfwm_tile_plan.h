// Watermark-tile preparation, the part that needs no HIP: Pillow's LANCZOS coefficient table of
// one axis, the per-byte arithmetic of the two resample passes, and the plan of a ragged call
// (tmfwm_prepare_tiles_ragged): N jobs, each with its own watermark and tile size, through one
// table upload and one set of launches.  Plain C++: a host compiler builds the plan
// and walks the two grids with the same functions the kernels run (tests/native/tile_plan_host.cpp).
#pragma once
#include <stdint.h>

#include <cmath>
#include <map>
#include <utility>
#include <vector>

#if defined(__HIPCC__)
#define TMF_HD __host__ __device__ __forceinline__
#else
#define TMF_HD inline
#endif

namespace tmf {

constexpr int kPrecisionBits = 32 - 8 - 2;

namespace tile_detail {

inline double sinc(double x)
{
    if (x == 0.0) return 1.0;
    x = x * 3.14159265358979323846;  // M_PI
    return std::sin(x) / x;
}

inline double lanczos(double x) { return (-3.0 <= x && x < 3.0) ? sinc(x) * sinc(x / 3) : 0.0; }

}  // namespace tile_detail

struct ResampleAxis {
    int ksize = 0;
    std::vector<int> bounds;  // 2 per output sample: first input index, count
    std::vector<int> kk;      // ksize 22-bit fixed-point taps per output sample
    void build(int in_size, int out_size);
};

// Resample.c precompute_coeffs + normalize_coeffs_8bpc for box (0, in_size) -> out_size.
inline void ResampleAxis::build(int in_size, int out_size)
{
    using tile_detail::lanczos;
    const float in0 = 0.0f, in1 = (float)in_size;
    double filterscale, scale;
    filterscale = scale = (double)(in1 - in0) / out_size;
    if (filterscale < 1.0) filterscale = 1.0;
    const double support = 3.0 * filterscale;
    ksize = (int)std::ceil(support) * 2 + 1;
    bounds.assign((size_t)out_size * 2, 0);
    kk.assign((size_t)out_size * ksize, 0);
    std::vector<double> k((size_t)ksize);
    for (int xx = 0; xx < out_size; xx++) {
        const double center = in0 + (xx + 0.5) * scale, ss = 1.0 / filterscale;
        double ww = 0.0;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        int x;
        for (x = 0; x < xmax; x++) {
            const double w = lanczos((x + xmin - center + 0.5) * ss);
            k[x] = w;
            ww += w;
        }
        for (x = 0; x < xmax; x++)
            if (ww != 0.0) k[x] /= ww;
        for (; x < ksize; x++) k[x] = 0;
        for (x = 0; x < ksize; x++)
            kk[(size_t)xx * ksize + x] =
                k[x] < 0 ? (int)(-0.5 + k[x] * (1 << kPrecisionBits)) : (int)(0.5 + k[x] * (1 << kPrecisionBits));
        bounds[xx * 2] = xmin;
        bounds[xx * 2 + 1] = xmax;
    }
}

// ---- the per-byte arithmetic of the two passes (every resample kernel and the host check)

TMF_HD uint8_t clip8(int v)
{
    v >>= kPrecisionBits;
    return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

// horizontal: clip8(2^21 + sum_x src[x] * k[x]); src = the input row at the sample's first input
// index, k = its taps (either may be a pointer into another address space)
template <class Src, class Taps>
TMF_HD uint8_t resample_h_byte(Src src, Taps k, int xmax)
{
    int ss = 1 << (kPrecisionBits - 1);
    for (int x = 0; x < xmax; x++) ss += (int)src[x] * k[x];
    return clip8(ss);
}

// vertical: clip8(2^21 + sum_y in[ymin + y][xx] * k[y]) over an input of row length iw
template <class Src, class Taps>
TMF_HD uint8_t resample_v_byte(Src in, int iw, int xx, int ymin, Taps k, int ymax)
{
    int ss = 1 << (kPrecisionBits - 1);
    for (int y = 0; y < ymax; y++) ss += (int)in[(int64_t)(y + ymin) * iw + xx] * k[y];
    return clip8(ss);
}

// ---- the ragged call

// Row segment of the two ragged grids: one work item (one workgroup of kTileSeg threads) writes
// kTileSeg consecutive bytes of one row.  A wave's width: the tiles of the app's frames are 80 to
// 240 bytes wide at b = 8, and a 256-wide segment would leave most of a workgroup idle on them.
#ifndef TMF_TILE_SEG
#define TMF_TILE_SEG 64  // -DTMF_TILE_SEG=256 builds the other width (the A/B of DESIGN.md 6)
#endif
constexpr int kTileSeg = TMF_TILE_SEG;

// One job as the kernels see it (device memory, read through the constant address space).
struct TileJob {
    const uint8_t *wm;  // ih x iw grey bytes
    uint8_t *tile;      // th x tw
    int64_t scratch;    // need_h: offset of its `rows` x rw intermediate rows in the group's scratch
    int32_t ih, iw;
    int32_t rh, rw;     // the resized watermark (the whole tile without preserve_ratio)
    int32_t th, tw;
    int32_t px, py;     // where the resized watermark is pasted; the rest of the tile is 255
    int32_t y_first, rows;  // the input rows [y_first, y_first + rows) the vertical filter reads
    int32_t need_h, need_v;  // rw != iw, rh != ih
    // this job's two axes in the packed table buffer (offsets in ints): bounds, taps, taps per sample.
    // An axis is shared by every job and direction with its (in, out) sizes, so the vertical bounds
    // are not rebased: the kernel subtracts y_first where it reads the intermediate rows.
    int32_t h_bounds, h_kk, h_ksize;
    int32_t v_bounds, v_kk, v_ksize;
    // exclusive prefix sums over the group's jobs of the two passes' work items (row segments):
    uint32_t h_item0;   // rows * ceil(rw / kTileSeg) per job with need_h
    uint32_t v_item0;   // th * ceil(tw / kTileSeg) per job
};
static_assert(sizeof(TileJob) == 104, "tile job table entry");

TMF_HD int tile_segs(int w) { return (w + kTileSeg - 1) / kTileSeg; }

// the job that owns work item x of a pass: the last i in [0, n) with prefix(i) <= x (a job without
// work in the pass shares its successor's prefix and is never found)
template <class Prefix>
TMF_HD int tile_find(int n, uint32_t x, Prefix prefix)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((uint32_t)prefix(mid) <= x) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// Horizontal pass, thread `lane` of work item `item` (relative to the job): one byte of the
// intermediate rows [y_first, y_first + rows) x rw.  J: a job (any address space), tables: the
// packed tables, scratch: the group's scratch.
template <class Job, class Tables>
TMF_HD void tile_h_thread(Job *J, uint32_t item, int lane, Tables tables, uint8_t *scratch)
{
    const int rw = J->rw, segs = tile_segs(rw);
    const int yy = (int)(item / (uint32_t)segs), xx = (int)(item % (uint32_t)segs) * kTileSeg + lane;
    if (xx >= rw) return;
    const int iw = J->iw;
    const auto bounds = tables + J->h_bounds;
    const int xmin = bounds[2 * xx], xmax = bounds[2 * xx + 1];
    const uint8_t *src = J->wm + (int64_t)(yy + J->y_first) * iw + xmin;
    scratch[J->scratch + (int64_t)yy * rw + xx] = resample_h_byte(src, tables + J->h_kk + (int64_t)xx * J->h_ksize, xmax);
}

// Vertical pass and paste, thread `lane` of work item `item` (relative to the job): one byte of
// the th x tw tile -- 255 outside the paste rectangle; inside it the vertical taps over the
// intermediate rows (need_h) or the watermark, or a copy of them (no need_v).
template <class Job, class Tables>
TMF_HD void tile_v_thread(Job *J, uint32_t item, int lane, Tables tables, const uint8_t *scratch)
{
    const int tw = J->tw, segs = tile_segs(tw);
    const int ty = (int)(item / (uint32_t)segs), tx = (int)(item % (uint32_t)segs) * kTileSeg + lane;
    if (tx >= tw) return;
    uint8_t *out = J->tile + (int64_t)ty * tw + tx;
    const int ry = ty - J->py, rx = tx - J->px, rw = J->rw;
    if (ry < 0 || ry >= J->rh || rx < 0 || rx >= rw) {
        *out = 255;
        return;
    }
    // the rows the vertical filter reads: the intermediate rows, which start at input row y_first,
    // or the watermark itself (rw == iw then)
    const bool h = J->need_h != 0;
    const uint8_t *src = h ? scratch + J->scratch : J->wm;
    const int y0 = h ? J->y_first : 0;
    if (J->need_v) {
        const auto bounds = tables + J->v_bounds;
        const int ymin = bounds[2 * ry] - y0, ymax = bounds[2 * ry + 1];
        *out = resample_v_byte(src, rw, rx, ymin, tables + J->v_kk + (int64_t)ry * J->v_ksize, ymax);
    } else {
        *out = src[(int64_t)(ry - y0) * rw + rx];
    }
}

// ---- its plan (host)

// resize_watermark's geometry (watermarking.py:105-123): the resized size and the paste offsets of
// a wh x ww watermark on a th x tw tile.  false: the resized size is empty (PIL raises there).
struct TileGeom {
    int rh, rw, px, py;
};

inline bool tile_geom(int wh, int ww, int th, int tw, bool preserve_ratio, TileGeom &g)
{
    g = TileGeom{th, tw, 0, 0};
    if (!preserve_ratio) return true;
    const double fw = (double)tw / (double)ww, fh = (double)th / (double)wh;
    const double ratio = fh < fw ? fh : fw;  // Python min() keeps the first of equals
    g.rw = (int)((double)ww * ratio);
    g.rh = (int)((double)wh * ratio);
    if (g.rw <= 0 || g.rh <= 0) return false;
    g.px = (tw - g.rw) / 2;  // :120-121
    g.py = (th - g.rh) / 2;
    return true;
}

struct TileJobIn {
    const uint8_t *wm;
    uint8_t *tile;
    int32_t wh, ww, th, tw;
};

// Jobs [first, first + n) of the table run as one pair of launches.
struct TileGroup {
    int64_t first = 0, n = 0;
    int64_t h_items = 0, v_items = 0;  // the two grids (h_items == 0: no horizontal launch)
    int64_t scratch = 0;               // bytes of intermediate rows
};

// Default bound of a group's scratch: the largest realistic job (a 300 x 300 QR code to a 4K
// frame's 480-wide tile) keeps 300 rows x 480 bytes = 144 KB, so 64 MB holds a few hundred of them.
constexpr int64_t kTileScratchCap = int64_t(64) << 20;
constexpr int64_t kTileItemCap = (int64_t(1) << 31) - 1;  // work items of one launch (prefixes are 32-bit)

struct TilePlan {
    std::vector<TileJob> jobs;
    std::vector<int> tables;  // every distinct axis once: [bounds | kk] each
    std::vector<TileGroup> groups;
    int64_t scratch = 0;      // the largest group's: the groups run in stream order and share it
    int axes = 0;             // distinct (in, out) axes built

    // -1: planned.  i >= 0: job i cannot be planned (*why says what).  The sizes are > 0.
    int64_t build(const TileJobIn *in, int64_t n, bool preserve_ratio, int64_t scratch_cap, const char **why);

private:
    struct AxisRef {
        int32_t bounds, kk, ksize, first, last;  // input samples [first, last) feed the axis
    };
    std::map<std::pair<int, int>, AxisRef> axes_;
    bool axis(int in_size, int out_size, AxisRef &r);
};

// the axis (in, out), built and packed on first use; false: the tables outgrow 32-bit offsets
inline bool TilePlan::axis(int in_size, int out_size, AxisRef &r)
{
    const auto key = std::make_pair(in_size, out_size);
    const auto it = axes_.find(key);
    if (it != axes_.end()) {
        r = it->second;
        return true;
    }
    // ksize as build() has it, before the table is made
    const double fs = (double)((float)in_size) / out_size;
    const int64_t ks = (int64_t)std::ceil(3.0 * (fs < 1.0 ? 1.0 : fs)) * 2 + 1;
    if ((int64_t)tables.size() + (int64_t)out_size * (2 + ks) > 0x7FFFFFFFll) return false;
    ResampleAxis a;
    a.build(in_size, out_size);
    r.bounds = (int32_t)tables.size();
    tables.insert(tables.end(), a.bounds.begin(), a.bounds.end());
    r.kk = (int32_t)tables.size();
    tables.insert(tables.end(), a.kk.begin(), a.kk.end());
    r.ksize = a.ksize;
    r.first = a.bounds[0];
    r.last = a.bounds[(size_t)out_size * 2 - 2] + a.bounds[(size_t)out_size * 2 - 1];
    axes_.emplace(key, r);
    ++axes;
    return true;
}

inline int64_t TilePlan::build(const TileJobIn *in, int64_t n, bool preserve_ratio, int64_t scratch_cap, const char **why)
{
    TileGroup g;
    for (int64_t i = 0; i < n; ++i) {
        const TileJobIn &s = in[i];
        TileGeom geo;
        if (!tile_geom(s.wh, s.ww, s.th, s.tw, preserve_ratio, geo)) {
            *why = "the resized watermark is empty";
            return i;
        }
        TileJob j{};
        j.wm = s.wm;
        j.tile = s.tile;
        j.ih = s.wh;
        j.iw = s.ww;
        j.rh = geo.rh;
        j.rw = geo.rw;
        j.th = s.th;
        j.tw = s.tw;
        j.px = geo.px;
        j.py = geo.py;
        j.need_h = j.rw != j.iw;
        j.need_v = j.rh != j.ih;
        AxisRef h, v;
        if (!axis(j.iw, j.rw, h) || !axis(j.ih, j.rh, v)) {
            *why = "the resample tables of the call exceed 2^31 entries";
            return i;
        }
        j.h_bounds = h.bounds;
        j.h_kk = h.kk;
        j.h_ksize = h.ksize;
        j.v_bounds = v.bounds;
        j.v_kk = v.kk;
        j.v_ksize = v.ksize;
        j.y_first = v.first;  // as ResamplePlan::build: the rows the vertical filter uses
        j.rows = v.last - v.first;
        const int64_t h_items = j.need_h ? (int64_t)j.rows * tile_segs(j.rw) : 0;
        const int64_t v_items = (int64_t)j.th * tile_segs(j.tw);
        const int64_t tmp = j.need_h ? (int64_t)j.rows * j.rw : 0;
        if (h_items > kTileItemCap || v_items > kTileItemCap) {
            *why = "more than 2^31 - 1 row segments";
            return i;
        }
        if (g.n > 0 && (g.scratch + tmp > scratch_cap || g.h_items + h_items > kTileItemCap || g.v_items + v_items > kTileItemCap)) {
            groups.push_back(g);
            if (g.scratch > scratch) scratch = g.scratch;
            g = TileGroup{};
            g.first = i;
        }
        j.scratch = g.scratch;
        j.h_item0 = (uint32_t)g.h_items;
        j.v_item0 = (uint32_t)g.v_items;
        jobs.push_back(j);
        ++g.n;
        g.h_items += h_items;
        g.v_items += v_items;
        g.scratch += tmp;
    }
    if (g.n > 0) {
        groups.push_back(g);
        if (g.scratch > scratch) scratch = g.scratch;
    }
    return -1;
}

}  // namespace tmf
