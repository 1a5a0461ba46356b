// C ABI of libtmfwm.so (declared in include/tmfwm.h): argument checking, host
// staging for TMFWM_MEM_HOST, stream selection and error reporting around the
// kernel launchers of tmfwm_kernels.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/tmfwm.h"
#include "tmfwm_internal.h"
#include "tmfwm_ragged.h"

namespace {

thread_local std::string t_err;
thread_local int64_t t_list_pass = -1;  // tmfwm_last_list_pass_blocks

int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    t_err = buf;
    return code;
}

#define TMF_HIP(call)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (call);                                                                         \
        if (e_ != hipSuccess) return fail(TMFWM_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)

hipStream_t pick_stream(void *s) { return s ? reinterpret_cast<hipStream_t>(s) : hipStreamPerThread; }

bool supported_block(int b) { return b >= 4 && b <= 16 && b % 2 == 0; }  // the UI slider values

// A device pointer handed in as TMFWM_MEM_DEVICE must really be device memory:
// a host pointer dereferenced by a kernel would fault the GPU.
int check_device_ptr(const void *p, const char *name)
{
    if (p == nullptr) return fail(TMFWM_ERR_INVALID, "%s is NULL", name);
    hipPointerAttribute_t at;
    hipError_t e = hipPointerGetAttributes(&at, p);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(TMFWM_ERR_INVALID, "%s is not a HIP device pointer (%s)", name, hipGetErrorString(e));
    }
    if (at.type != hipMemoryTypeDevice && at.type != hipMemoryTypeManaged)
        return fail(TMFWM_ERR_INVALID, "%s is not device memory (memory type %d)", name, (int)at.type);
    return 0;
}

// The library's own stream-ordered pool per device (never the device's default pool, which
// torch's allocator and other libraries share): freed blocks stay cached up to kPoolKeep
// bytes -- enough for the per-call dgesdd lists and the host path's staging of an app-sized
// call -- and anything above is returned to the device at the next synchronisation.
constexpr uint64_t kPoolKeep = uint64_t(1) << 30;

hipMemPool_t lib_pool(int dev)
{
    static std::mutex mu;
    static std::vector<std::pair<int, hipMemPool_t>> pools;
    std::lock_guard<std::mutex> lk(mu);
    for (auto &p : pools)
        if (p.first == dev) return p.second;
    hipMemPoolProps props{};
    props.allocType = hipMemAllocationTypePinned;
    props.handleTypes = hipMemHandleTypeNone;
    props.location.type = hipMemLocationTypeDevice;
    props.location.id = dev;
    hipMemPool_t pool = nullptr;
    if (hipMemPoolCreate(&pool, &props) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    uint64_t keep = kPoolKeep;
    (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep);
    pools.emplace_back(dev, pool);
    return pool;
}

// the device a stream belongs to (the null / per-thread stream: the current device)
int stream_device(hipStream_t st)
{
    int dev = 0;
    if (st != nullptr && st != hipStreamPerThread) {
        hipDevice_t d = 0;
        if (hipStreamGetDevice(st, &d) == hipSuccess) return (int)d;
        (void)hipGetLastError();
    }
    if (hipGetDevice(&dev) != hipSuccess) (void)hipGetLastError();
    return dev;
}

// Device scratch for one call, stream-ordered from the library's pool on the stream's
// device, released (stream-ordered) in the destructor.
struct DevBuf {
    void *p = nullptr;
    hipStream_t st = nullptr;
    ~DevBuf()
    {
        if (p) (void)hipFreeAsync(p, st);
    }
    int alloc(size_t n, hipStream_t s, const char *what)
    {
        st = s;
        if (n == 0) return 0;
        hipMemPool_t pool = lib_pool(stream_device(s));
        hipError_t e = pool ? hipMallocFromPoolAsync(&p, n, pool, s) : hipMallocAsync(&p, n, s);
        if (e != hipSuccess) {
            p = nullptr;
            (void)hipGetLastError();
            return fail(TMFWM_ERR_NOMEM, "device allocation of %zu bytes for %s failed: %s", n, what, hipGetErrorString(e));
        }
        return 0;
    }
};

int check_frames(int64_t n, int32_t H, int32_t W, int64_t stride, int32_t block)
{
    if (n < 0 || H < 0 || W < 0) return fail(TMFWM_ERR_INVALID, "negative size (n=%lld, H=%d, W=%d)", (long long)n, H, W);
    if (!supported_block(block)) return fail(TMFWM_ERR_UNSUPPORTED, "block size %d not supported (even, 4..16)", block);
    if (stride < (int64_t)H * W * 3) return fail(TMFWM_ERR_INVALID, "frame_stride %lld < H*W*3", (long long)stride);
    return 0;
}

// check_frames for frames of px bytes per pixel (the keyed *_px entries): 3 is check_frames itself
int check_frames_px(int64_t n, int32_t H, int32_t W, int32_t px, int64_t stride, int32_t block)
{
    if (px == TMFWM_PIX_RGB) return check_frames(n, H, W, stride, block);
    if (px != TMFWM_PIX_RGBX) return fail(TMFWM_ERR_INVALID, "pixel bytes %d (3 or 4)", px);
    if (int rc = check_frames(n, H, W, (int64_t)H * W * 3, block)) return rc;
    if (stride < (int64_t)H * W * 4) return fail(TMFWM_ERR_INVALID, "frame_stride %lld < H*W*4", (long long)stride);
    return 0;
}

// After argument validation: there is no CPU fallback, so no device is an error.
int need_device()
{
    int dev = 0;
    if (hipGetDeviceCount(&dev) != hipSuccess || dev == 0) {
        (void)hipGetLastError();
        return fail(TMFWM_ERR_NODEVICE, "no HIP device available");
    }
    return 0;
}

// [a, a+na) and [b, b+nb) share a byte (the kernels read one while writing the other)
bool ranges_overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return na && nb && x < y + nb && y < x + na;
}

size_t span_bytes(int64_t n, int64_t stride, int64_t frame_bytes) { return n == 0 ? 0 : (size_t)((n - 1) * stride + frame_bytes); }

// tile_stride of the per-frame-tile calls: 0 (one shared tile) or at least a tile (padded tiles are allowed)
int check_tile_stride(int64_t tile_stride, int64_t tbytes)
{
    if (tile_stride < 0 || (tile_stride != 0 && tile_stride < tbytes))
        return fail(TMFWM_ERR_INVALID, "tile_stride %lld: 0 (one shared tile) or >= (H/block)*(W/block) = %lld", (long long)tile_stride,
                    (long long)tbytes);
    return 0;
}

// n items of `bytes` each, `stride` bytes apart in host memory (0: one item shared by all), to or
// from compact device memory in one copy; the caller's bytes between the items are not touched.
size_t item_count(int64_t n, int64_t stride) { return stride ? (size_t)n : 1; }

int copy_items(void *dev, const void *host, size_t bytes, int64_t n, int64_t stride, hipMemcpyKind kind, hipStream_t st)
{
    const size_t count = item_count(n, stride);
    const bool up = kind == hipMemcpyHostToDevice;
    void *dst = up ? dev : const_cast<void *>(host);
    const void *src = up ? host : dev;
    if (bytes == 0) return 0;
    if (count == 1 || stride == (int64_t)bytes)
        TMF_HIP(hipMemcpyAsync(dst, src, bytes * count, kind, st));
    else
        TMF_HIP(hipMemcpy2DAsync(dst, up ? bytes : (size_t)stride, src, up ? (size_t)stride : bytes, bytes, count, kind, st));
    return 0;
}

// Host tiles (tile_stride apart; 0: one tile) staged into `buf`; *dstride is the stride the
// kernels then use.
int stage_tiles(const uint8_t *tiles, int64_t n, int64_t tile_stride, size_t tbytes, hipStream_t st, DevBuf &buf, const uint8_t **dev,
                int64_t *dstride)
{
    if (int rc = buf.alloc(tbytes * item_count(n, tile_stride), st, "watermark tiles")) return rc;
    if (int rc = copy_items(buf.p, tiles, tbytes, n, tile_stride, hipMemcpyHostToDevice, st)) return rc;
    *dev = static_cast<const uint8_t *>(buf.p);
    *dstride = tile_stride ? (int64_t)tbytes : 0;
    return 0;
}

// Second-pass bookkeeping: frames go in chunks of at most kListCap
// blocks (and 65535 frames, the grid's y limit); each chunk's first pass appends the
// blocks that need the dgesdd route to one shared id list (u32, chunk-relative) and
// counts them in its own slot of `counts`; its fixup pass runs right after it on the
// same stream.  The fixup pass is latency-bound (one serial dgesdd per thread, a few ms
// whatever the list length), so chunks are made as large as the list allows:
// kListCap = 2^29 ids = 2 GiB (4 bytes per block, 2 % of the frames' own bytes at b = 8),
// i.e. 4142 4K frames at b = 8 -- configs[2] / [3] take one chunk per GPU.
// TMFWM_DEBUG_LIST_CAP (ids) lowers it so that the tests can exercise several chunks.
constexpr int64_t kListCap = int64_t(1) << 29;

// TMFWM_DEBUG_FORCE_NONCONV=1 marks one dgesdd-route block of every chunk as not converged
// (tests: the non-convergence report of the synchronising calls, include/tmfwm.h)
bool force_nonconv()
{
    const char *e = std::getenv("TMFWM_DEBUG_FORCE_NONCONV");
    return e && *e && *e != '0';
}

int64_t list_cap()
{
    const char *e = std::getenv("TMFWM_DEBUG_LIST_CAP");
    if (!e || !*e) return kListCap;
    const long long v = std::atoll(e);
    return v > 0 && v < kListCap ? (int64_t)v : kListCap;
}

struct Chunks {
    int64_t per_frame = 0, frames = 0, n = 0, cap = 0, total = 0;
    int64_t first(int64_t c) const { return c * frames; }  // chunk c: frames [first, first + count)
    int64_t count(int64_t c) const { return std::min(frames, total - c * frames); }
    std::vector<int64_t> blocks() const  // per chunk, for two_pass
    {
        std::vector<int64_t> b((size_t)n);
        for (int64_t c = 0; c < n; ++c) b[(size_t)c] = count(c) * per_frame;
        return b;
    }
    void plan(int64_t nframes, int64_t blocks_per_frame)
    {
        total = nframes;
        per_frame = blocks_per_frame;
        frames = blocks_per_frame > 0 ? list_cap() / blocks_per_frame : nframes;
        if (frames < 1) frames = 1;
        if (frames > 65535) frames = 65535;
        if (frames > nframes) frames = nframes;
        n = frames > 0 ? (nframes + frames - 1) / frames : 0;
        cap = frames * blocks_per_frame;
    }
};

// sum the per-chunk counts h[0 .. 3*nchunks) (dgesdd-route, non-convergence, list-pass)
int sum_host_counts(const uint32_t *h, int64_t nchunks, int64_t *out)
{
    int64_t t = 0, bad = 0, slow = 0;
    for (int64_t c = 0; c < nchunks; ++c) {
        t += h[c];
        bad += h[nchunks + c];
        slow += h[2 * nchunks + c];
    }
    if (out) *out = t;
    t_list_pass = slow;
    if (bad)
        return fail(TMFWM_ERR_HIP, "dgesdd route: dbdsqr did not converge on %lld block(s) (np.linalg.svd raises LinAlgError there)",
                    (long long)bad);
    return 0;
}

// copy the per-chunk counts back (synchronises the stream) and sum them
int sum_counts(const uint32_t *dcounts, int64_t nchunks, hipStream_t st, int64_t *out)
{
    std::vector<uint32_t> h((size_t)(3 * nchunks));
    if (nchunks) {
        hipError_t e = hipMemcpyAsync(h.data(), dcounts, (size_t)nchunks * 12, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) {
            t_list_pass = -1;
            return fail(TMFWM_ERR_HIP, "reading the dgesdd-route counts failed: %s", hipGetErrorString(e));
        }
    }
    return sum_host_counts(h.data(), nchunks, out);
}

// Pinned landing zones for the per-chunk counts of host-memory calls: the counts travel with the
// call's last copy and are read after its one synchronisation (no extra round trip between the
// kernels and the copy back).  A small process-wide free list, so no thread keeps pinned memory.
constexpr int64_t kSinkChunks = 16;
std::mutex g_sink_mu;
std::vector<uint32_t *> g_sinks;

struct HostSink {
    uint32_t *p = nullptr;
    hipStream_t st = nullptr;
    HostSink(int64_t nchunks, hipStream_t s) : st(s)
    {
        if (nchunks > kSinkChunks) return;  // the synchronous read-back instead
        {
            std::lock_guard<std::mutex> g(g_sink_mu);
            if (!g_sinks.empty()) {
                p = g_sinks.back();
                g_sinks.pop_back();
                return;
            }
        }
        if (hipHostMalloc(reinterpret_cast<void **>(&p), kSinkChunks * 12, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            p = nullptr;
        }
    }
    ~HostSink()
    {
        if (!p) return;
        (void)hipStreamSynchronize(st);  // an error return may leave the copy into it in flight
        (void)hipGetLastError();
        std::lock_guard<std::mutex> g(g_sink_mu);
        g_sinks.push_back(p);
    }
    HostSink(const HostSink &) = delete;
    HostSink &operator=(const HostSink &) = delete;
};

// ---- the two-pass driver: the bookkeeping above, once, for every batch call

// The lists and counters of one chunk, under the names the kernels' argument structs give them.
struct ChunkLists {
    uint32_t *fb_list, *fb_count, *fb_bad;           // dgesdd route: ids, how many, how many did not converge
    uint32_t *slow_list, *slow_count, *slow_shards;  // list pass (list and shards null: the call has none)
};

template <class Args>  // EmbedArgs, ExtractArgs, KeyedArgs: the same six fields
void wire_lists(Args &k, const ChunkLists &w)
{
    k.fb_list = w.fb_list;
    k.fb_count = w.fb_count;
    k.fb_bad = w.fb_bad;
    k.slow_list = w.slow_list;
    k.slow_count = w.slow_count;
    k.slow_shards = w.slow_shards;
}

// Where a call's per-chunk counts (dgesdd-route blocks, dbdsqr non-convergence, list-pass blocks)
// go.  They are read back -- which synchronises the stream -- when the caller asks for the count
// (n_lapack) or when `check` is set (the host-memory calls, which synchronise anyway): a dbdsqr
// that did not converge then fails the call (np.linalg.svd raises LinAlgError there).  With a
// `sink` they are copied there on the stream instead and nothing synchronises here: whoever owns
// the sink sums it after its own synchronisation (HostCall, tmf::embed_device_async).  An
// asynchronous device-memory call without a count pointer is not checked (include/tmfwm.h).
struct Report {
    int64_t *n_lapack;
    bool check;
    uint32_t *sink;
};

// Both passes of a call whose chunks hold blocks[c] blocks each.  enqueue(c, lists) launches
// chunk c's first pass (or launch_list_all) and then its fixup pass on `st`, with `lists` wired
// into its argument struct; here, around it: the allocations, the zeroed counts, the reset of the
// segment counters before each chunk, the TMFWM_DEBUG_FORCE_NONCONV poke after it (chunks with
// a block only) and the report.
//   list_pass    allocate the list-pass list and its segment counters (else the kernels get null)
//   edge_chunks  ragged: a chunk may hold edge pixels and no block, and is enqueued all the same;
//                without it a call with no block anywhere reports zero counts at once and
//                allocates nothing
template <class Enqueue>
int two_pass(const std::vector<int64_t> &blocks, bool list_pass, bool edge_chunks, hipStream_t st, const Report &rep, Enqueue enqueue)
{
    const int64_t nch = (int64_t)blocks.size();
    const int64_t cap = nch ? *std::max_element(blocks.begin(), blocks.end()) : 0;  // ids are relative to the chunk
    if (cap == 0 && !edge_chunks) {
        if (rep.sink) std::fill(rep.sink, rep.sink + 3 * nch, 0u);
        if (rep.n_lapack) {
            *rep.n_lapack = 0;
            t_list_pass = 0;
        }
        return 0;
    }
    DevBuf list, slow, shards, counts;
    const size_t shard_bytes = (size_t)tmf::kListShards * tmf::kShardStride * 4;
    if (int rc = list.alloc((size_t)cap * 4, st, "dgesdd-route block list")) return rc;
    if (list_pass) {
        if (int rc = slow.alloc((size_t)cap * 4, st, "list-pass block list")) return rc;
        if (int rc = shards.alloc(shard_bytes, st, "list-pass segment counters")) return rc;
    }
    // per chunk: dgesdd-route count, non-convergence count, list-pass count
    if (int rc = counts.alloc((size_t)nch * 12, st, "block-list counts")) return rc;
    TMF_HIP(hipMemsetAsync(counts.p, 0, (size_t)nch * 12, st));
    uint32_t *const cnt = static_cast<uint32_t *>(counts.p);
    for (int64_t c = 0; c < nch; ++c) {
        const ChunkLists w{static_cast<uint32_t *>(list.p), cnt + c,           cnt + nch + c,
                           static_cast<uint32_t *>(slow.p), cnt + 2 * nch + c, static_cast<uint32_t *>(shards.p)};
        if (shards.p) TMF_HIP(hipMemsetAsync(shards.p, 0, shard_bytes, st));
        if (int rc = enqueue(c, w)) return rc;
        if (blocks[(size_t)c] > 0 && force_nonconv()) TMF_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(w.fb_bad), 1, 1, st));
    }
    if (rep.sink) {
        TMF_HIP(hipMemcpyAsync(rep.sink, counts.p, (size_t)nch * 12, hipMemcpyDeviceToHost, st));
        return 0;
    }
    if (rep.n_lapack || rep.check) return sum_counts(cnt, nch, st, rep.n_lapack);
    return 0;
}

// ---- the call shell of the batch entry points

// Every batch entry point starts here.  A route outside the enumeration leaves *n_lapack as the
// caller had it; from the zeroing on, an early return leaves this call's counts at 0.
int begin_call(int32_t route, int64_t *n_lapack, bool rank1_routes = true)
{
    t_err.clear();
    if (route < TMFWM_ROUTE_HYBRID || route > TMFWM_ROUTE_RANK1_REFERENCE) return fail(TMFWM_ERR_INVALID, "route %d", route);
    if (!rank1_routes && (route == TMFWM_ROUTE_RANK1 || route == TMFWM_ROUTE_RANK1_REFERENCE))
        return fail(TMFWM_ERR_UNSUPPORTED, "the ragged calls do not take the rank-1 routes yet (route %d)", route);
    if (n_lapack) {
        *n_lapack = 0;
        t_list_pass = 0;
    }
    return 0;
}

// The frame of a host-memory call, made once its inputs are staged: it takes a sink, the passes
// run with report() -- their counts go to the sink; without one (more than kSinkChunks chunks)
// they read the counts back themselves -- the caller enqueues the copies of its results, and
// finish() synchronises the one time and sums the sink.
struct HostCall {
    HostSink sink;
    int64_t nchunks, *n_lapack;
    HostCall(int64_t nch, hipStream_t st, int64_t *n) : sink(nch, st), nchunks(nch), n_lapack(n) {}
    Report report() const { return {n_lapack, true, sink.p}; }
    int finish()
    {
        TMF_HIP(hipStreamSynchronize(sink.st));
        return sink.p && nchunks ? tmf::sum_sink(sink.p, nchunks, n_lapack) : 0;
    }
};

// a device-memory call has no sink: it reads the counts back if the caller gave a count pointer
Report device_report(int64_t *n_lapack) { return {n_lapack, false, nullptr}; }

}  // namespace

namespace tmf {
int report(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    t_err = buf;
    return code;
}

void clear_error() { t_err.clear(); }

int check_frames(int64_t n, int32_t H, int32_t W, int64_t stride, int32_t block) { return ::check_frames(n, H, W, stride, block); }

// the embed call also wants the key (a.key_out) and its passes do not store it themselves: on the
// rank-1 routes (the pre-pass is not fused) and at a size whose key variant is not built
// (tmfwm_embed_key.h) the call runs the map's passes after the embed's
bool embed_key_composed(int block, int route, bool key)
{
    const bool pre = (route == TMFWM_ROUTE_RANK1 || route == TMFWM_ROUTE_RANK1_REFERENCE) && rank1_block(block);
    return key && (pre || !embed_key_fused(block));
}

KeyedArgs keyed_args(int64_t n, int32_t H, int32_t W, int64_t stride, int32_t block, double alpha);
bool dev_aligned(const void *p, const void *q, int64_t stride, int W);

// Both passes of embed over device-resident frames (a.src / a.dst / a.wm set).  With a.key_out
// the key of the frames in a.src as well: out of the key variants of the same
// passes, or -- composed -- by the map's passes over chunks of their own after the embed's, on
// the same stream and through the same driver, so that the counts are the sums over both.
int run_embed(const EmbedArgs &a, hipStream_t st, const Report &rep, int route)
{
    Chunks ch;
    ch.plan(a.nframes, (int64_t)a.nbh * a.nbw);
    if (ch.cap == 0) TMF_HIP(launch_embed(a, st));  // no full block: the colour round trip only, zero counts, no key entry
    const bool pre = (route == TMFWM_ROUTE_RANK1 || route == TMFWM_ROUTE_RANK1_REFERENCE) && rank1_block(a.block);
    const bool embed_list = (embed_defers(a.block) && route != TMFWM_ROUTE_REFERENCE && route != TMFWM_ROUTE_RANK1_REFERENCE) ||
                            (route == TMFWM_ROUTE_RANK1 && pre);
    const bool composed = embed_key_composed(a.block, route, a.key_out != nullptr);
    std::vector<int64_t> blocks = ch.blocks();
    if (composed) blocks.insert(blocks.end(), blocks.begin(), blocks.begin() + ch.n);  // the map's chunks
    const bool map_list = composed && route != TMFWM_ROUTE_REFERENCE;
    return two_pass(blocks, embed_list || map_list, false, st, rep, [&](int64_t cc, const ChunkLists &w) -> int {
        const int64_t c = cc % ch.n, f0 = ch.first(c), nb = ch.count(c) * ch.per_frame;
        if (cc >= ch.n) {  // composed: tmfwm_sigma1_map's passes over the chunk (run_keyed)
            KeyedArgs m = keyed_args(ch.count(c), a.H, a.W, a.frame_stride, a.block, 1.0);
            m.src = a.src + f0 * a.frame_stride;
            m.key_out = a.key_out + f0 * a.key_stride;
            m.key_stride = a.key_stride;
            m.aligned = dev_aligned(m.src, m.src, a.frame_stride, a.W);
            wire_lists(m, w);
            if (route == TMFWM_ROUTE_REFERENCE) TMF_HIP(launch_list_all(m.fb_list, m.fb_count, nb, st));
            else TMF_HIP(launch_sigma1_map(m, st));
            TMF_HIP(launch_sigma1_fixup(m, m.fb_list, m.fb_count, nb, st));
            return 0;
        }
        EmbedArgs k = a;
        k.nframes = ch.count(c);
        k.src = a.src + f0 * a.frame_stride;
        k.dst = a.dst + f0 * a.frame_stride;
        k.wm = a.wm + f0 * a.wm_stride;  // the lists' block ids are relative to the chunk: so is its first tile
        k.key_out = a.key_out && !composed ? a.key_out + f0 * a.key_stride : nullptr;  // ... and its first key
        wire_lists(k, w);
        if (!embed_list) k.slow_list = k.slow_shards = nullptr;  // (allocated for the map's chunks)
        if (route == TMFWM_ROUTE_REFERENCE || (route == TMFWM_ROUTE_RANK1_REFERENCE && !pre)) {
            // every block on the dgesdd route; the edges as always
            TMF_HIP(launch_edges(k.src, k.dst, k.nframes, k.H, k.W, k.frame_stride, k.block, st));
            TMF_HIP(launch_list_all(k.fb_list, k.fb_count, nb, st));
        } else if (pre) {  // the rank-1 pre-pass (+ its list pass for TMFWM_ROUTE_RANK1), the edges
            if (route == TMFWM_ROUTE_RANK1_REFERENCE) k.slow_list = nullptr;
            TMF_HIP(launch_embed_rank1(k, st));
        } else {
            TMF_HIP(launch_embed(k, st));
        }
        TMF_HIP(launch_embed_fixup(k, k.fb_list, k.fb_count, nb, st));
        return 0;
    });
}

int run_extract(const ExtractArgs &a, hipStream_t st, const Report &rep, int route)
{
    Chunks ch;
    ch.plan(a.nframes, (int64_t)a.nbh * a.nbw);
    // the list pass on every route but the reference (TMFWM_ROUTE_RANK1: extract is the hybrid route)
    return two_pass(ch.blocks(), route != TMFWM_ROUTE_REFERENCE, false, st, rep, [&](int64_t c, const ChunkLists &w) -> int {
        ExtractArgs k = a;
        const int64_t f0 = ch.first(c), nb = ch.count(c) * ch.per_frame;
        k.nframes = ch.count(c);
        k.wsrc = a.wsrc + f0 * a.frame_stride;
        k.osrc = a.osrc + f0 * a.frame_stride;
        k.out = a.out + f0 * a.tile_stride;
        wire_lists(k, w);
        if (route == TMFWM_ROUTE_REFERENCE) TMF_HIP(launch_list_all(k.fb_list, k.fb_count, nb, st));
        else TMF_HIP(launch_extract(k, st));
        TMF_HIP(launch_extract_fixup(k, k.fb_list, k.fb_count, nb, st));
        return 0;
    });
}

// Keyed extraction over device-resident frames (a.src, and a.key_out for the map or a.key / a.out
// for the extract, set): as run_extract, on one image per frame of px bytes per pixel.
int run_keyed(const KeyedArgs &a, bool map, hipStream_t st, const Report &rep, int route, int px = 3)
{
    Chunks ch;
    ch.plan(a.nframes, (int64_t)a.nbh * a.nbw);
    return two_pass(ch.blocks(), route != TMFWM_ROUTE_REFERENCE, false, st, rep, [&](int64_t c, const ChunkLists &w) -> int {
        KeyedArgs k = a;
        const int64_t f0 = ch.first(c), nb = ch.count(c) * ch.per_frame;
        k.nframes = ch.count(c);
        k.src = a.src + f0 * a.frame_stride;
        if (map) k.key_out = a.key_out + f0 * a.key_stride;
        else {
            k.key = a.key + f0 * a.key_stride;  // stride 0: the one shared key
            k.out = a.out + f0 * a.tile_stride;
        }
        wire_lists(k, w);
        if (route == TMFWM_ROUTE_REFERENCE) TMF_HIP(launch_list_all(k.fb_list, k.fb_count, nb, st));
        else TMF_HIP(map ? launch_sigma1_map(k, st, px) : launch_extract_keyed(k, st, px));
        TMF_HIP(map ? launch_sigma1_fixup(k, k.fb_list, k.fb_count, nb, st, px)
                    : launch_extract_keyed_fixup(k, k.fb_list, k.fb_count, nb, st, px));
        return 0;
    });
}

// the geometry every launch struct carries
template <class Args>
Args geometry(int64_t n, int32_t H, int32_t W, int64_t stride, int32_t block)
{
    Args a{};
    a.nframes = n;
    a.frame_stride = stride;
    a.H = H;
    a.W = W;
    a.block = block;
    a.nbh = H / block;
    a.nbw = W / block;
    return a;
}

EmbedArgs embed_args(int64_t n, int32_t H, int32_t W, int64_t stride, int32_t block, double alpha)
{
    EmbedArgs a = geometry<EmbedArgs>(n, H, W, stride, block);
    a.alpha = alpha;
    return a;
}

ExtractArgs extract_args(int64_t n, int32_t H, int32_t W, int64_t stride, int32_t block, double alpha)
{
    ExtractArgs a = geometry<ExtractArgs>(n, H, W, stride, block);
    a.tile_stride = (int64_t)a.nbh * a.nbw;
    a.alpha32 = (float)alpha;
    return a;
}

KeyedArgs keyed_args(int64_t n, int32_t H, int32_t W, int64_t stride, int32_t block, double alpha)
{
    KeyedArgs a = geometry<KeyedArgs>(n, H, W, stride, block);
    a.tile_stride = (int64_t)a.nbh * a.nbw;
    a.key_stride = a.tile_stride;
    a.alpha32 = (float)alpha;
    return a;
}

bool dev_aligned(const void *p, const void *q, int64_t stride, int W)
{
    return ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(q)) % 4 == 0) && stride % 4 == 0 && W % 4 == 0;
}

// KeyedArgs::aligned of frames of px bytes per pixel: at 4 every pixel is a dword once the base
// and the frame stride are multiples of 4, whatever W is
bool keyed_aligned(const void *p, int64_t stride, int W, int px)
{
    return px == 4 ? reinterpret_cast<uintptr_t>(p) % 4 == 0 && stride % 4 == 0 : dev_aligned(p, p, stride, W);
}

int64_t count_chunks(int64_t nframes, int H, int W, int block)
{
    Chunks ch;
    ch.plan(nframes, (int64_t)(H / block) * (W / block));
    return ch.n;
}

int embed_device_async(const uint8_t *src, int64_t n, int H, int W, int64_t stride, const uint8_t *tile, int64_t tile_stride,
                       int block, double alpha, uint8_t *dst, hipStream_t st, uint32_t *sink, int route)
{
    if (int rc = ::check_frames(n, H, W, stride, block)) return rc;
    if (n == 0 || H == 0 || W == 0) {
        std::fill(sink, sink + 3 * count_chunks(n, H, W, block), 0u);
        return 0;
    }
    EmbedArgs a = embed_args(n, H, W, stride, block, alpha);
    a.src = src;
    a.dst = dst;
    a.wm = tile;
    a.wm_stride = tile_stride;
    a.aligned = dev_aligned(src, dst, stride, W);
    return run_embed(a, st, Report{nullptr, false, sink}, route);
}

int extract_device_async(const uint8_t *wsrc, const uint8_t *osrc, int64_t n, int H, int W, int64_t stride, int block,
                         double alpha, uint8_t *out, hipStream_t st, uint32_t *sink, int route)
{
    if (int rc = ::check_frames(n, H, W, stride, block)) return rc;
    if (n == 0 || (H / block) * (W / block) == 0) {
        std::fill(sink, sink + 3 * count_chunks(n, H, W, block), 0u);
        return 0;
    }
    ExtractArgs a = extract_args(n, H, W, stride, block, alpha);
    a.wsrc = wsrc;
    a.osrc = osrc;
    a.out = out;
    a.aligned = dev_aligned(wsrc, osrc, stride, W);
    return run_extract(a, st, Report{nullptr, false, sink}, route);
}

int sum_sink(const uint32_t *sink, int64_t nchunks, int64_t *lapack) { return sum_host_counts(sink, nchunks, lapack); }
}  // namespace tmf

extern "C" {

int tmfwm_abi_version(void) { return TMFWM_ABI_VERSION; }

const char *tmfwm_last_error(void) { return t_err.c_str(); }

int64_t tmfwm_last_list_pass_blocks(void) { return t_list_pass; }

int tmfwm_embed_list_pass(int32_t block) { return supported_block(block) && tmf::embed_defers(block) ? 1 : 0; }

int tmfwm_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

// 3-byte pixels in and out, one frame stride (tmfwm_embed_route; tmfwm_embed_tiles' 3 -> 3 case;
// tmfwm_embed_key): frame f's tile at wm_tile + f * tile_stride (0: one tile for every frame);
// with_key: frame f's key to out_key + f * key_stride bytes
static int embed_rgb(const uint8_t *rgb, int64_t n_frames, int32_t height, int32_t width, int64_t frame_stride,
                     const uint8_t *wm_tile, int64_t tile_stride, int32_t block, double alpha, uint8_t *out, int32_t mem_kind,
                     void *hip_stream, int32_t route, int64_t *n_lapack_blocks, bool with_key = false, float *out_key = nullptr,
                     int64_t key_stride = 0, bool px_entry = false)
{
    if (int rc = begin_call(route, n_lapack_blocks)) return rc;
    if (int rc = check_frames(n_frames, height, width, frame_stride, block)) return rc;
    const int nbh = height / block, nbw = width / block;
    if (int rc = check_tile_stride(tile_stride, (int64_t)nbh * nbw)) return rc;
    if (!std::isfinite(alpha)) return fail(TMFWM_ERR_INVALID, "alpha is not finite");
    const int64_t kbytes = (int64_t)nbh * nbw * 4;
    if (with_key && n_frames > 1 && (key_stride % 4 != 0 || key_stride < kbytes))
        return fail(TMFWM_ERR_INVALID, "key_stride %lld: a multiple of 4 >= (H/block)*(W/block)*4 = %lld", (long long)key_stride,
                    (long long)kbytes);
    // (tmfwm_embed_key_px checks the key pointer's alignment before the device is looked for)
    if (px_entry && with_key && kbytes > 0 && reinterpret_cast<uintptr_t>(out_key) % 4) return fail(TMFWM_ERR_INVALID, "out_key is not 4-byte aligned");
    if (int rc = need_device()) return rc;
    if (n_frames == 0 || height == 0 || width == 0) return 0;
    with_key = with_key && kbytes > 0;  // no block: the colour round trip and no key entry
    if (n_frames == 1) key_stride = kbytes;
    const int64_t fbytes = (int64_t)height * width * 3;
    const size_t span = span_bytes(n_frames, frame_stride, fbytes), tbytes = (size_t)nbh * nbw;
    const size_t tspan = span_bytes(n_frames, tile_stride, (int64_t)tbytes);  // every frame's tile
    const size_t kspan = with_key ? (size_t)((n_frames - 1) * key_stride + kbytes) : 0;
    hipStream_t st = pick_stream(hip_stream);
    tmf::EmbedArgs a = tmf::embed_args(n_frames, height, width, frame_stride, block, alpha);
    if (mem_kind == TMFWM_MEM_DEVICE) {
        if (int rc = check_device_ptr(rgb, "rgb")) return rc;
        if (int rc = check_device_ptr(out, "out")) return rc;
        if (tbytes) {
            if (int rc = check_device_ptr(wm_tile, "wm_tile")) return rc;
        }
        if (ranges_overlap(rgb, span, out, span)) return fail(TMFWM_ERR_INVALID, "out overlaps rgb (in-place embed is not supported)");
        if (tbytes && ranges_overlap(wm_tile, tspan, out, span)) return fail(TMFWM_ERR_INVALID, "out overlaps wm_tile");
        if (with_key) {
            if (int rc = check_device_ptr(out_key, "out_key")) return rc;
            if (reinterpret_cast<uintptr_t>(out_key) % 4) return fail(TMFWM_ERR_INVALID, "out_key is not 4-byte aligned");
            if (ranges_overlap(out_key, kspan, rgb, span) || ranges_overlap(out_key, kspan, wm_tile, tspan))
                return fail(TMFWM_ERR_INVALID, "out_key's output overlaps an input of the call");
            if (ranges_overlap(out_key, kspan, out, span)) return fail(TMFWM_ERR_INVALID, "out_key's output overlaps out");
            a.key_out = out_key;
            a.key_stride = key_stride / 4;
        }
        a.src = rgb;
        a.dst = out;
        a.wm = wm_tile;
        a.wm_stride = tile_stride;
        a.aligned = tmf::dev_aligned(rgb, out, frame_stride, width);
        return tmf::run_embed(a, st, device_report(n_lapack_blocks), route);
    }
    if (mem_kind != TMFWM_MEM_HOST) return fail(TMFWM_ERR_INVALID, "mem_kind %d", mem_kind);
    if (!rgb || !out || (tbytes && !wm_tile) || (with_key && !out_key)) return fail(TMFWM_ERR_INVALID, "NULL host pointer");
    if (with_key && reinterpret_cast<uintptr_t>(out_key) % 4) return fail(TMFWM_ERR_INVALID, "out_key is not 4-byte aligned");
    DevBuf din, dout, dwm, dkey;
    if (int rc = din.alloc(span, st, "input frames")) return rc;
    if (int rc = dout.alloc(span, st, "output frames")) return rc;
    if (with_key) {  // staged compact
        if (int rc = dkey.alloc((size_t)(kbytes * n_frames), st, "sigma_1 key maps")) return rc;
        a.key_out = static_cast<float *>(dkey.p);
        a.key_stride = kbytes / 4;
    }
    TMF_HIP(hipMemcpyAsync(din.p, rgb, span, hipMemcpyHostToDevice, st));
    if (int rc = stage_tiles(wm_tile, n_frames, tile_stride, tbytes, st, dwm, &a.wm, &a.wm_stride)) return rc;
    a.src = static_cast<const uint8_t *>(din.p);
    a.dst = static_cast<uint8_t *>(dout.p);
    a.aligned = frame_stride % 4 == 0 && width % 4 == 0;
    const int64_t nch = tmf::count_chunks(n_frames, height, width, block);
    HostCall hc(tmf::embed_key_composed(block, route, with_key) ? 2 * nch : nch, st, n_lapack_blocks);
    if (int rc = tmf::run_embed(a, st, hc.report(), route)) return rc;
    if (frame_stride == fbytes) {
        TMF_HIP(hipMemcpyAsync(out, dout.p, span, hipMemcpyDeviceToHost, st));
    } else {
        for (int64_t f = 0; f < n_frames; ++f)
            TMF_HIP(hipMemcpyAsync(out + f * frame_stride, static_cast<uint8_t *>(dout.p) + f * frame_stride, (size_t)fbytes,
                                   hipMemcpyDeviceToHost, st));
    }
    if (with_key) {  // as the frames: one copy, or one per frame past the caller's padding
        const uint8_t *dk = static_cast<const uint8_t *>(dkey.p);
        if (key_stride == kbytes) {
            TMF_HIP(hipMemcpyAsync(out_key, dk, (size_t)(kbytes * n_frames), hipMemcpyDeviceToHost, st));
        } else {
            for (int64_t f = 0; f < n_frames; ++f)
                TMF_HIP(hipMemcpyAsync(reinterpret_cast<uint8_t *>(out_key) + f * key_stride, dk + f * kbytes, (size_t)kbytes,
                                       hipMemcpyDeviceToHost, st));
        }
    }
    return hc.finish();
}

int tmfwm_embed_key(const uint8_t *rgb, int64_t n_frames, int32_t height, int32_t width, int64_t frame_stride,
                    const uint8_t *wm_tiles, int64_t tile_stride, int32_t block, double alpha, uint8_t *out, float *out_key,
                    int64_t key_stride, int32_t mem_kind, void *hip_stream, int32_t route, int64_t *n_lapack_blocks)
{
    return embed_rgb(rgb, n_frames, height, width, frame_stride, wm_tiles, tile_stride, block, alpha, out, mem_kind, hip_stream, route,
                     n_lapack_blocks, true, out_key, key_stride);
}

int tmfwm_embed_route(const uint8_t *rgb, int64_t n_frames, int32_t height, int32_t width, int64_t frame_stride,
                      const uint8_t *wm_tile, int32_t block, double alpha, uint8_t *out, int32_t mem_kind, void *hip_stream,
                      int32_t route, int64_t *n_lapack_blocks)
{
    return embed_rgb(rgb, n_frames, height, width, frame_stride, wm_tile, 0, block, alpha, out, mem_kind, hip_stream, route,
                     n_lapack_blocks);
}

int tmfwm_embed_ex(const uint8_t *rgb, int64_t n_frames, int32_t height, int32_t width, int64_t frame_stride,
                   const uint8_t *wm_tile, int32_t block, double alpha, uint8_t *out, int32_t mem_kind, void *hip_stream,
                   int64_t *n_lapack_blocks)
{
    return tmfwm_embed_route(rgb, n_frames, height, width, frame_stride, wm_tile, block, alpha, out, mem_kind, hip_stream,
                             TMFWM_ROUTE_HYBRID, n_lapack_blocks);
}

int tmfwm_embed(const uint8_t *rgb, int64_t n_frames, int32_t height, int32_t width, int64_t frame_stride,
                const uint8_t *wm_tile, int32_t block, double alpha, uint8_t *out, int32_t mem_kind, void *hip_stream)
{
    return tmfwm_embed_ex(rgb, n_frames, height, width, frame_stride, wm_tile, block, alpha, out, mem_kind, hip_stream, nullptr);
}

int tmfwm_extract_route(const uint8_t *wm_rgb, const uint8_t *orig_rgb, int64_t n_frames, int32_t height, int32_t width,
                        int64_t frame_stride, int32_t block, double alpha, uint8_t *out_tiles, int32_t mem_kind,
                        void *hip_stream, int32_t route, int64_t *n_lapack_blocks)
{
    if (int rc = begin_call(route, n_lapack_blocks)) return rc;
    if (int rc = check_frames(n_frames, height, width, frame_stride, block)) return rc;
    if (!std::isfinite(alpha) || alpha == 0.0) return fail(TMFWM_ERR_INVALID, "alpha must be finite and non-zero");
    if (int rc = need_device()) return rc;
    const int nbh = height / block, nbw = width / block;
    const int64_t tbytes = (int64_t)nbh * nbw;
    if (n_frames == 0 || tbytes == 0) return 0;
    const int64_t fbytes = (int64_t)height * width * 3;
    const size_t span = span_bytes(n_frames, frame_stride, fbytes);
    hipStream_t st = pick_stream(hip_stream);
    tmf::ExtractArgs a = tmf::extract_args(n_frames, height, width, frame_stride, block, alpha);
    if (mem_kind == TMFWM_MEM_DEVICE) {
        if (int rc = check_device_ptr(wm_rgb, "wm_rgb")) return rc;
        if (int rc = check_device_ptr(orig_rgb, "orig_rgb")) return rc;
        if (int rc = check_device_ptr(out_tiles, "out_tiles")) return rc;
        const size_t obytes = (size_t)(tbytes * n_frames);
        if (ranges_overlap(out_tiles, obytes, wm_rgb, span) || ranges_overlap(out_tiles, obytes, orig_rgb, span))
            return fail(TMFWM_ERR_INVALID, "out_tiles overlaps an input batch");
        a.wsrc = wm_rgb;
        a.osrc = orig_rgb;
        a.out = out_tiles;
        a.aligned = tmf::dev_aligned(wm_rgb, orig_rgb, frame_stride, width);
        return tmf::run_extract(a, st, device_report(n_lapack_blocks), route);
    }
    if (mem_kind != TMFWM_MEM_HOST) return fail(TMFWM_ERR_INVALID, "mem_kind %d", mem_kind);
    if (!wm_rgb || !orig_rgb || !out_tiles) return fail(TMFWM_ERR_INVALID, "NULL host pointer");
    DevBuf dw, dor, dout;
    if (int rc = dw.alloc(span, st, "watermarked frames")) return rc;
    if (int rc = dor.alloc(span, st, "original frames")) return rc;
    if (int rc = dout.alloc((size_t)(tbytes * n_frames), st, "extracted tiles")) return rc;
    TMF_HIP(hipMemcpyAsync(dw.p, wm_rgb, span, hipMemcpyHostToDevice, st));
    TMF_HIP(hipMemcpyAsync(dor.p, orig_rgb, span, hipMemcpyHostToDevice, st));
    a.wsrc = static_cast<const uint8_t *>(dw.p);
    a.osrc = static_cast<const uint8_t *>(dor.p);
    a.out = static_cast<uint8_t *>(dout.p);
    a.aligned = frame_stride % 4 == 0 && width % 4 == 0;
    HostCall hc(tmf::count_chunks(n_frames, height, width, block), st, n_lapack_blocks);
    if (int rc = tmf::run_extract(a, st, hc.report(), route)) return rc;
    TMF_HIP(hipMemcpyAsync(out_tiles, dout.p, (size_t)(tbytes * n_frames), hipMemcpyDeviceToHost, st));
    return hc.finish();
}

int tmfwm_extract_ex(const uint8_t *wm_rgb, const uint8_t *orig_rgb, int64_t n_frames, int32_t height, int32_t width,
                     int64_t frame_stride, int32_t block, double alpha, uint8_t *out_tiles, int32_t mem_kind, void *hip_stream,
                     int64_t *n_lapack_blocks)
{
    return tmfwm_extract_route(wm_rgb, orig_rgb, n_frames, height, width, frame_stride, block, alpha, out_tiles, mem_kind,
                               hip_stream, TMFWM_ROUTE_HYBRID, n_lapack_blocks);
}

int tmfwm_extract(const uint8_t *wm_rgb, const uint8_t *orig_rgb, int64_t n_frames, int32_t height, int32_t width,
                  int64_t frame_stride, int32_t block, double alpha, uint8_t *out_tiles, int32_t mem_kind, void *hip_stream)
{
    return tmfwm_extract_ex(wm_rgb, orig_rgb, n_frames, height, width, frame_stride, block, alpha, out_tiles, mem_kind,
                            hip_stream, nullptr);
}

// ---- keyed extraction (within ABI 10): the original's per-block f32 sigma_1 as a key
// frames of px bytes per pixel, read where they lie (tmfwm_sigma1_map: 3; tmfwm_sigma1_map_px, which
// also checks out_key's alignment before the device is looked for: px_entry)
static int sigma1_map_frames(const uint8_t *rgb, int32_t px, int64_t n_frames, int32_t height, int32_t width, int64_t frame_stride,
                             int32_t block, float *out_key, int32_t mem_kind, void *hip_stream, int32_t route,
                             int64_t *n_lapack_blocks, bool px_entry)
{
    if (int rc = begin_call(route, n_lapack_blocks)) return rc;
    if (int rc = check_frames_px(n_frames, height, width, px, frame_stride, block)) return rc;
    if (px_entry && reinterpret_cast<uintptr_t>(out_key) % 4) return fail(TMFWM_ERR_INVALID, "out_key is not 4-byte aligned");
    if (int rc = need_device()) return rc;
    const int64_t kbytes = (int64_t)(height / block) * (width / block) * 4;
    if (n_frames == 0 || kbytes == 0) return 0;
    const size_t span = span_bytes(n_frames, frame_stride, (int64_t)height * width * px), obytes = (size_t)(kbytes * n_frames);
    hipStream_t st = pick_stream(hip_stream);
    tmf::KeyedArgs a = tmf::keyed_args(n_frames, height, width, frame_stride, block, 1.0);
    if (mem_kind == TMFWM_MEM_DEVICE) {
        if (int rc = check_device_ptr(rgb, "rgb")) return rc;
        if (int rc = check_device_ptr(out_key, "out_key")) return rc;
        if (reinterpret_cast<uintptr_t>(out_key) % 4) return fail(TMFWM_ERR_INVALID, "out_key is not 4-byte aligned");
        if (ranges_overlap(out_key, obytes, rgb, span)) return fail(TMFWM_ERR_INVALID, "out_key overlaps the input batch");
        a.src = rgb;
        a.key_out = out_key;
        a.aligned = tmf::keyed_aligned(rgb, frame_stride, width, px);
        return tmf::run_keyed(a, true, st, device_report(n_lapack_blocks), route, px);
    }
    if (mem_kind != TMFWM_MEM_HOST) return fail(TMFWM_ERR_INVALID, "mem_kind %d", mem_kind);
    if (!rgb || !out_key) return fail(TMFWM_ERR_INVALID, "NULL host pointer");
    DevBuf din, dkey;
    if (int rc = din.alloc(span, st, "frames")) return rc;
    if (int rc = dkey.alloc(obytes, st, "sigma_1 key maps")) return rc;
    TMF_HIP(hipMemcpyAsync(din.p, rgb, span, hipMemcpyHostToDevice, st));
    a.src = static_cast<const uint8_t *>(din.p);
    a.key_out = static_cast<float *>(dkey.p);
    a.aligned = tmf::keyed_aligned(din.p, frame_stride, width, px);  // (the staging buffer is aligned)
    HostCall hc(tmf::count_chunks(n_frames, height, width, block), st, n_lapack_blocks);
    if (int rc = tmf::run_keyed(a, true, st, hc.report(), route, px)) return rc;
    TMF_HIP(hipMemcpyAsync(out_key, dkey.p, obytes, hipMemcpyDeviceToHost, st));
    return hc.finish();
}

int tmfwm_sigma1_map(const uint8_t *rgb, int64_t n_frames, int32_t height, int32_t width, int64_t frame_stride, int32_t block,
                     float *out_key, int32_t mem_kind, void *hip_stream, int32_t route, int64_t *n_lapack_blocks)
{
    return sigma1_map_frames(rgb, TMFWM_PIX_RGB, n_frames, height, width, frame_stride, block, out_key, mem_kind, hip_stream, route,
                             n_lapack_blocks, false);
}

int tmfwm_sigma1_map_px(const uint8_t *rgb, int32_t pixel_bytes, int64_t frame_stride, int64_t n_frames, int32_t height,
                        int32_t width, int32_t block, float *out_key, int32_t mem_kind, void *hip_stream, int32_t route,
                        int64_t *n_lapack_blocks)
{
    return sigma1_map_frames(rgb, pixel_bytes, n_frames, height, width, frame_stride, block, out_key, mem_kind, hip_stream, route,
                             n_lapack_blocks, true);
}

static int extract_keyed_frames(const uint8_t *wm_rgb, int32_t px, int64_t n_frames, int32_t height, int32_t width,
                                int64_t frame_stride, const float *key, int64_t key_stride, int32_t block, double alpha,
                                uint8_t *out_tiles, int32_t mem_kind, void *hip_stream, int32_t route, int64_t *n_lapack_blocks,
                                bool px_entry)
{
    if (int rc = begin_call(route, n_lapack_blocks)) return rc;
    if (int rc = check_frames_px(n_frames, height, width, px, frame_stride, block)) return rc;
    if (!std::isfinite(alpha) || alpha == 0.0) return fail(TMFWM_ERR_INVALID, "alpha must be finite and non-zero");
    const int64_t tbytes = (int64_t)(height / block) * (width / block), kbytes = tbytes * 4;
    if (key_stride < 0 || key_stride % 4 != 0 || (key_stride != 0 && key_stride < kbytes))
        return fail(TMFWM_ERR_INVALID, "key_stride %lld: 0 (one shared key) or a multiple of 4 >= (H/block)*(W/block)*4 = %lld",
                    (long long)key_stride, (long long)kbytes);
    if (px_entry && reinterpret_cast<uintptr_t>(key) % 4) return fail(TMFWM_ERR_INVALID, "key is not 4-byte aligned");
    if (int rc = need_device()) return rc;
    if (n_frames == 0 || tbytes == 0) return 0;
    const size_t span = span_bytes(n_frames, frame_stride, (int64_t)height * width * px), obytes = (size_t)(tbytes * n_frames);
    const size_t kspan = (size_t)((key_stride ? (n_frames - 1) * key_stride : 0) + kbytes);
    hipStream_t st = pick_stream(hip_stream);
    tmf::KeyedArgs a = tmf::keyed_args(n_frames, height, width, frame_stride, block, alpha);
    if (mem_kind == TMFWM_MEM_DEVICE) {
        if (int rc = check_device_ptr(wm_rgb, "wm_rgb")) return rc;
        if (int rc = check_device_ptr(key, "key")) return rc;
        if (int rc = check_device_ptr(out_tiles, "out_tiles")) return rc;
        if (reinterpret_cast<uintptr_t>(key) % 4) return fail(TMFWM_ERR_INVALID, "key is not 4-byte aligned");
        if (ranges_overlap(out_tiles, obytes, wm_rgb, span) || ranges_overlap(out_tiles, obytes, key, kspan))
            return fail(TMFWM_ERR_INVALID, "out_tiles overlaps an input");
        a.src = wm_rgb;
        a.key = key;
        a.key_stride = key_stride / 4;
        a.out = out_tiles;
        a.aligned = tmf::keyed_aligned(wm_rgb, frame_stride, width, px);
        return tmf::run_keyed(a, false, st, device_report(n_lapack_blocks), route, px);
    }
    if (mem_kind != TMFWM_MEM_HOST) return fail(TMFWM_ERR_INVALID, "mem_kind %d", mem_kind);
    if (!wm_rgb || !key || !out_tiles) return fail(TMFWM_ERR_INVALID, "NULL host pointer");
    DevBuf dw, dkey, dout;
    if (int rc = dw.alloc(span, st, "watermarked frames")) return rc;
    if (int rc = dkey.alloc((size_t)kbytes * item_count(n_frames, key_stride), st, "sigma_1 key maps")) return rc;  // staged compact
    if (int rc = dout.alloc(obytes, st, "extracted tiles")) return rc;
    TMF_HIP(hipMemcpyAsync(dw.p, wm_rgb, span, hipMemcpyHostToDevice, st));
    if (int rc = copy_items(dkey.p, key, (size_t)kbytes, n_frames, key_stride, hipMemcpyHostToDevice, st)) return rc;
    a.src = static_cast<const uint8_t *>(dw.p);
    a.key = static_cast<const float *>(dkey.p);
    a.key_stride = key_stride ? tbytes : 0;
    a.out = static_cast<uint8_t *>(dout.p);
    a.aligned = tmf::keyed_aligned(dw.p, frame_stride, width, px);  // (the staging buffer is aligned)
    HostCall hc(tmf::count_chunks(n_frames, height, width, block), st, n_lapack_blocks);
    if (int rc = tmf::run_keyed(a, false, st, hc.report(), route, px)) return rc;
    TMF_HIP(hipMemcpyAsync(out_tiles, dout.p, obytes, hipMemcpyDeviceToHost, st));
    return hc.finish();
}

int tmfwm_extract_keyed(const uint8_t *wm_rgb, int64_t n_frames, int32_t height, int32_t width, int64_t frame_stride,
                        const float *key, int64_t key_stride, int32_t block, double alpha, uint8_t *out_tiles, int32_t mem_kind,
                        void *hip_stream, int32_t route, int64_t *n_lapack_blocks)
{
    return extract_keyed_frames(wm_rgb, TMFWM_PIX_RGB, n_frames, height, width, frame_stride, key, key_stride, block, alpha, out_tiles,
                                mem_kind, hip_stream, route, n_lapack_blocks, false);
}

int tmfwm_extract_keyed_px(const uint8_t *wm_rgb, int32_t pixel_bytes, int64_t frame_stride, int64_t n_frames, int32_t height,
                           int32_t width, const float *key, int64_t key_stride, int32_t block, double alpha, uint8_t *out_tiles,
                           int32_t mem_kind, void *hip_stream, int32_t route, int64_t *n_lapack_blocks)
{
    return extract_keyed_frames(wm_rgb, pixel_bytes, n_frames, height, width, frame_stride, key, key_stride, block, alpha, out_tiles,
                                mem_kind, hip_stream, route, n_lapack_blocks, true);
}

// ---- 4-byte pixels (ABI 8): the core runs on compact RGB device buffers; RGBX inputs are
// packed and RGBX outputs unpacked on the device (tmfwm_pixels.hip)
extern "C++" {
namespace {
int check_px(int32_t px, int64_t stride, int32_t H, int32_t W, const char *what)
{
    if (px != TMFWM_PIX_RGB && px != TMFWM_PIX_RGBX) return fail(TMFWM_ERR_INVALID, "%s pixel bytes %d (3 or 4)", what, px);
    if (stride < (int64_t)H * W * px) return fail(TMFWM_ERR_INVALID, "%s frame_stride %lld < H*W*%d", what, (long long)stride, px);
    return 0;
}

// frames (host or device, 3 or 4 bytes per pixel) -> device RGB with stride *s3; buf / tmp own
// whatever had to be allocated
int device_rgb(const uint8_t *src, int32_t px, int64_t stride, int64_t n, int32_t H, int32_t W, int32_t mem_kind,
               hipStream_t st, const char *what, DevBuf &buf, DevBuf &tmp, const uint8_t **out, int64_t *s3)
{
    const int64_t f3 = (int64_t)H * W * 3;
    const size_t span = span_bytes(n, stride, (int64_t)H * W * px);
    const uint8_t *p = src;
    if (mem_kind == TMFWM_MEM_DEVICE) {
        if (int rc = check_device_ptr(src, what)) return rc;
    } else {
        if (!src) return fail(TMFWM_ERR_INVALID, "NULL host pointer (%s)", what);
        if (int rc = (px == 3 ? buf : tmp).alloc(span, st, what)) return rc;
        p = static_cast<const uint8_t *>((px == 3 ? buf : tmp).p);
        TMF_HIP(hipMemcpyAsync(const_cast<uint8_t *>(p), src, span, hipMemcpyHostToDevice, st));
    }
    if (px == 3) {
        *out = p;
        *s3 = stride;
        return 0;
    }
    if (int rc = buf.alloc((size_t)(n * f3), st, what)) return rc;
    TMF_HIP(tmf::launch_pack_rgbx(p, stride, static_cast<uint8_t *>(buf.p), f3, n, H, W, st));
    *out = static_cast<const uint8_t *>(buf.p);
    *s3 = f3;
    return 0;
}
}  // namespace
}  // extern "C++"

// tmfwm_embed_tiles, and with_key tmfwm_embed_key_px: frame f's key to out_key + f * key_stride bytes,
// out of the embed passes over the packed 3-byte frames (run_embed with a.key_out)
static int embed_layouts(const uint8_t *rgb, int32_t in_pixel_bytes, int64_t in_frame_stride, int64_t n_frames, int32_t height,
                         int32_t width, const uint8_t *wm_tiles, int64_t tile_stride, int32_t block, double alpha, uint8_t *out,
                         int32_t out_pixel_bytes, int64_t out_frame_stride, int32_t mem_kind, void *hip_stream, int32_t route,
                         int64_t *n_lapack_blocks, bool with_key, float *out_key, int64_t key_stride)
{
    t_err.clear();
    const uint8_t *wm_tile = wm_tiles;
    if (in_pixel_bytes == TMFWM_PIX_RGB && out_pixel_bytes == TMFWM_PIX_RGB) {
        if (in_frame_stride != out_frame_stride) return fail(TMFWM_ERR_INVALID, "3-byte input and output need one frame_stride");
        return embed_rgb(rgb, n_frames, height, width, in_frame_stride, wm_tile, tile_stride, block, alpha, out, mem_kind, hip_stream,
                         route, n_lapack_blocks, with_key, out_key, key_stride, with_key);
    }
    if (int rc = begin_call(route, n_lapack_blocks)) return rc;
    if (int rc = check_frames(n_frames, height, width, (int64_t)height * width * 3, block)) return rc;
    if (int rc = check_px(in_pixel_bytes, in_frame_stride, height, width, "input")) return rc;
    if (int rc = check_px(out_pixel_bytes, out_frame_stride, height, width, "output")) return rc;
    const int nbh = height / block, nbw = width / block;
    if (int rc = check_tile_stride(tile_stride, (int64_t)nbh * nbw)) return rc;
    if (!std::isfinite(alpha)) return fail(TMFWM_ERR_INVALID, "alpha is not finite");
    if (mem_kind != TMFWM_MEM_HOST && mem_kind != TMFWM_MEM_DEVICE) return fail(TMFWM_ERR_INVALID, "mem_kind %d", mem_kind);
    const int64_t kbytes = (int64_t)nbh * nbw * 4;
    if (with_key && n_frames > 1 && (key_stride % 4 != 0 || key_stride < kbytes))
        return fail(TMFWM_ERR_INVALID, "key_stride %lld: a multiple of 4 >= (H/block)*(W/block)*4 = %lld", (long long)key_stride,
                    (long long)kbytes);
    if (with_key && kbytes > 0 && reinterpret_cast<uintptr_t>(out_key) % 4) return fail(TMFWM_ERR_INVALID, "out_key is not 4-byte aligned");
    if (int rc = need_device()) return rc;
    if (n_frames == 0 || height == 0 || width == 0) return 0;
    with_key = with_key && kbytes > 0;  // no block: the colour round trip and no key entry
    if (n_frames == 1) key_stride = kbytes;
    const size_t kspan = with_key ? (size_t)((n_frames - 1) * key_stride + kbytes) : 0;
    const size_t tbytes = (size_t)nbh * nbw;
    const int64_t f3 = (int64_t)height * width * 3, fo = (int64_t)height * width * out_pixel_bytes;
    const size_t ospan = span_bytes(n_frames, out_frame_stride, fo);
    hipStream_t st = pick_stream(hip_stream);
    if (mem_kind == TMFWM_MEM_DEVICE) {
        if (int rc = check_device_ptr(out, "out")) return rc;
        if (ranges_overlap(rgb, span_bytes(n_frames, in_frame_stride, (int64_t)height * width * in_pixel_bytes), out, ospan))
            return fail(TMFWM_ERR_INVALID, "out overlaps rgb (in-place embed is not supported)");
        if (tbytes) {
            if (int rc = check_device_ptr(wm_tile, "wm_tile")) return rc;
            // per-frame tiles only: with one shared tile this is tmfwm_embed_px, which never had the rule
            if (tile_stride && ranges_overlap(wm_tile, span_bytes(n_frames, tile_stride, (int64_t)tbytes), out, ospan))
                return fail(TMFWM_ERR_INVALID, "out overlaps wm_tile");
        }
        if (with_key) {
            if (int rc = check_device_ptr(out_key, "out_key")) return rc;
            if (ranges_overlap(out_key, kspan, rgb, span_bytes(n_frames, in_frame_stride, (int64_t)height * width * in_pixel_bytes)) ||
                ranges_overlap(out_key, kspan, wm_tile, span_bytes(n_frames, tile_stride, (int64_t)tbytes)))
                return fail(TMFWM_ERR_INVALID, "out_key's output overlaps an input of the call");
            if (ranges_overlap(out_key, kspan, out, ospan)) return fail(TMFWM_ERR_INVALID, "out_key's output overlaps out");
        }
    } else if (!out || (tbytes && !wm_tile) || (with_key && !out_key)) {
        return fail(TMFWM_ERR_INVALID, "NULL host pointer");
    }
    DevBuf src3, tmp, dst3, dst4, dwm, dkey;
    const uint8_t *s3p = nullptr;
    int64_t s3 = 0;
    if (int rc = device_rgb(rgb, in_pixel_bytes, in_frame_stride, n_frames, height, width, mem_kind, st, "input frames", src3, tmp,
                            &s3p, &s3))
        return rc;
    const uint8_t *wm = wm_tile;
    int64_t wm_stride = tile_stride;
    if (mem_kind == TMFWM_MEM_HOST && tbytes) {
        if (int rc = stage_tiles(wm_tile, n_frames, tile_stride, tbytes, st, dwm, &wm, &wm_stride)) return rc;
    }
    if (int rc = dst3.alloc(span_bytes(n_frames, s3, f3), st, "output frames")) return rc;
    tmf::EmbedArgs a = tmf::embed_args(n_frames, height, width, s3, block, alpha);
    a.src = s3p;
    a.dst = static_cast<uint8_t *>(dst3.p);
    a.wm = wm;
    a.wm_stride = wm_stride;
    a.aligned = tmf::dev_aligned(a.src, a.dst, s3, width);
    if (with_key && mem_kind == TMFWM_MEM_DEVICE) {
        a.key_out = out_key;
        a.key_stride = key_stride / 4;
    } else if (with_key) {  // staged compact
        if (int rc = dkey.alloc((size_t)(kbytes * n_frames), st, "sigma_1 key maps")) return rc;
        a.key_out = static_cast<float *>(dkey.p);
        a.key_stride = kbytes / 4;
    }
    // the output's final layout (RGB or RGBX, the caller's stride) is made on the device, at `o`
    auto layout = [&](uint8_t *o) -> int {
        if (out_pixel_bytes == TMFWM_PIX_RGBX)
            TMF_HIP(tmf::launch_unpack_rgbx(a.dst, s3, o, out_frame_stride, n_frames, height, width, st));
        else
            TMF_HIP(hipMemcpy2DAsync(o, (size_t)out_frame_stride, a.dst, (size_t)s3, (size_t)f3, (size_t)n_frames,
                                     hipMemcpyDeviceToDevice, st));
        return 0;
    };
    if (mem_kind == TMFWM_MEM_DEVICE) {
        if (int rc = tmf::run_embed(a, st, device_report(n_lapack_blocks), route)) return rc;
        return layout(out);
    }
    const int64_t nch = tmf::count_chunks(n_frames, height, width, block);
    HostCall hc(tmf::embed_key_composed(block, route, with_key) ? 2 * nch : nch, st, n_lapack_blocks);
    if (int rc = tmf::run_embed(a, st, hc.report(), route)) return rc;
    if (int rc = dst4.alloc(ospan, st, "output staging")) return rc;
    if (int rc = layout(static_cast<uint8_t *>(dst4.p))) return rc;
    if (n_frames == 1 || out_frame_stride == fo)  // the caller's bytes between frames stay as they are
        TMF_HIP(hipMemcpyAsync(out, dst4.p, ospan, hipMemcpyDeviceToHost, st));
    else
        TMF_HIP(hipMemcpy2DAsync(out, (size_t)out_frame_stride, dst4.p, (size_t)out_frame_stride, (size_t)fo, (size_t)n_frames,
                                 hipMemcpyDeviceToHost, st));
    if (with_key)  // one copy, or one row per frame past the caller's padding
        TMF_HIP(hipMemcpy2DAsync(out_key, (size_t)key_stride, dkey.p, (size_t)kbytes, (size_t)kbytes, (size_t)n_frames,
                                 hipMemcpyDeviceToHost, st));
    return hc.finish();
}

int tmfwm_embed_tiles(const uint8_t *rgb, int32_t in_pixel_bytes, int64_t in_frame_stride, int64_t n_frames, int32_t height,
                      int32_t width, const uint8_t *wm_tiles, int64_t tile_stride, int32_t block, double alpha, uint8_t *out,
                      int32_t out_pixel_bytes, int64_t out_frame_stride, int32_t mem_kind, void *hip_stream, int32_t route,
                      int64_t *n_lapack_blocks)
{
    return embed_layouts(rgb, in_pixel_bytes, in_frame_stride, n_frames, height, width, wm_tiles, tile_stride, block, alpha, out,
                         out_pixel_bytes, out_frame_stride, mem_kind, hip_stream, route, n_lapack_blocks, false, nullptr, 0);
}

int tmfwm_embed_key_px(const uint8_t *rgb, int32_t in_pixel_bytes, int64_t in_frame_stride, int64_t n_frames, int32_t height,
                       int32_t width, const uint8_t *wm_tiles, int64_t tile_stride, int32_t block, double alpha, uint8_t *out,
                       int32_t out_pixel_bytes, int64_t out_frame_stride, float *out_key, int64_t key_stride, int32_t mem_kind,
                       void *hip_stream, int32_t route, int64_t *n_lapack_blocks)
{
    return embed_layouts(rgb, in_pixel_bytes, in_frame_stride, n_frames, height, width, wm_tiles, tile_stride, block, alpha, out,
                         out_pixel_bytes, out_frame_stride, mem_kind, hip_stream, route, n_lapack_blocks, true, out_key, key_stride);
}

int tmfwm_embed_px(const uint8_t *rgb, int32_t in_pixel_bytes, int64_t in_frame_stride, int64_t n_frames, int32_t height,
                   int32_t width, const uint8_t *wm_tile, int32_t block, double alpha, uint8_t *out, int32_t out_pixel_bytes,
                   int64_t out_frame_stride, int32_t mem_kind, void *hip_stream, int32_t route, int64_t *n_lapack_blocks)
{
    return tmfwm_embed_tiles(rgb, in_pixel_bytes, in_frame_stride, n_frames, height, width, wm_tile, 0, block, alpha, out,
                             out_pixel_bytes, out_frame_stride, mem_kind, hip_stream, route, n_lapack_blocks);
}

int tmfwm_extract_px(const uint8_t *wm_rgb, int32_t wm_pixel_bytes, int64_t wm_frame_stride, const uint8_t *orig_rgb,
                     int32_t orig_pixel_bytes, int64_t orig_frame_stride, int64_t n_frames, int32_t height, int32_t width,
                     int32_t block, double alpha, uint8_t *out_tiles, int32_t mem_kind, void *hip_stream, int32_t route,
                     int64_t *n_lapack_blocks)
{
    t_err.clear();
    if (wm_pixel_bytes == TMFWM_PIX_RGB && orig_pixel_bytes == TMFWM_PIX_RGB && wm_frame_stride == orig_frame_stride)
        return tmfwm_extract_route(wm_rgb, orig_rgb, n_frames, height, width, wm_frame_stride, block, alpha, out_tiles, mem_kind,
                                   hip_stream, route, n_lapack_blocks);
    if (int rc = begin_call(route, n_lapack_blocks)) return rc;
    if (int rc = check_frames(n_frames, height, width, (int64_t)height * width * 3, block)) return rc;
    if (int rc = check_px(wm_pixel_bytes, wm_frame_stride, height, width, "watermarked")) return rc;
    if (int rc = check_px(orig_pixel_bytes, orig_frame_stride, height, width, "original")) return rc;
    if (!std::isfinite(alpha) || alpha == 0.0) return fail(TMFWM_ERR_INVALID, "alpha must be finite and non-zero");
    if (mem_kind != TMFWM_MEM_HOST && mem_kind != TMFWM_MEM_DEVICE) return fail(TMFWM_ERR_INVALID, "mem_kind %d", mem_kind);
    if (int rc = need_device()) return rc;
    const int nbh = height / block, nbw = width / block;
    const int64_t tbytes = (int64_t)nbh * nbw, f3 = (int64_t)height * width * 3;
    if (n_frames == 0 || tbytes == 0) return 0;
    const size_t obytes = (size_t)(tbytes * n_frames);
    hipStream_t st = pick_stream(hip_stream);
    if (mem_kind == TMFWM_MEM_DEVICE) {
        if (int rc = check_device_ptr(out_tiles, "out_tiles")) return rc;
        if (ranges_overlap(out_tiles, obytes, wm_rgb, span_bytes(n_frames, wm_frame_stride, (int64_t)height * width * wm_pixel_bytes)) ||
            ranges_overlap(out_tiles, obytes, orig_rgb, span_bytes(n_frames, orig_frame_stride, (int64_t)height * width * orig_pixel_bytes)))
            return fail(TMFWM_ERR_INVALID, "out_tiles overlaps an input batch");
    } else if (!out_tiles) {
        return fail(TMFWM_ERR_INVALID, "NULL host pointer");
    }
    // both images as compact RGB (one frame stride for the kernels)
    DevBuf w3, wtmp, o3, otmp, wc, oc, dout;
    const uint8_t *wp = nullptr, *op = nullptr;
    int64_t ws = 0, os = 0;
    if (int rc = device_rgb(wm_rgb, wm_pixel_bytes, wm_frame_stride, n_frames, height, width, mem_kind, st, "watermarked frames", w3,
                            wtmp, &wp, &ws))
        return rc;
    if (int rc = device_rgb(orig_rgb, orig_pixel_bytes, orig_frame_stride, n_frames, height, width, mem_kind, st, "original frames",
                            o3, otmp, &op, &os))
        return rc;
    if (ws != f3) {
        if (int rc = wc.alloc((size_t)(n_frames * f3), st, "watermarked frames")) return rc;
        TMF_HIP(hipMemcpy2DAsync(wc.p, (size_t)f3, wp, (size_t)ws, (size_t)f3, (size_t)n_frames, hipMemcpyDeviceToDevice, st));
        wp = static_cast<const uint8_t *>(wc.p);
    }
    if (os != f3) {
        if (int rc = oc.alloc((size_t)(n_frames * f3), st, "original frames")) return rc;
        TMF_HIP(hipMemcpy2DAsync(oc.p, (size_t)f3, op, (size_t)os, (size_t)f3, (size_t)n_frames, hipMemcpyDeviceToDevice, st));
        op = static_cast<const uint8_t *>(oc.p);
    }
    tmf::ExtractArgs a = tmf::extract_args(n_frames, height, width, f3, block, alpha);
    a.wsrc = wp;
    a.osrc = op;
    if (mem_kind == TMFWM_MEM_HOST) {
        if (int rc = dout.alloc(obytes, st, "extracted tiles")) return rc;
        a.out = static_cast<uint8_t *>(dout.p);
    } else {
        a.out = out_tiles;
    }
    a.aligned = tmf::dev_aligned(wp, op, f3, width);
    if (mem_kind == TMFWM_MEM_DEVICE) return tmf::run_extract(a, st, device_report(n_lapack_blocks), route);
    HostCall hc(tmf::count_chunks(n_frames, height, width, block), st, n_lapack_blocks);
    if (int rc = tmf::run_extract(a, st, hc.report(), route)) return rc;
    TMF_HIP(hipMemcpyAsync(out_tiles, dout.p, obytes, hipMemcpyDeviceToHost, st));
    return hc.finish();
}

extern "C++" {
namespace {

// One elementwise colour helper: in_bytes / out_bytes per pixel; launch(in, out, st)
// on device pointers.  Host calls stage through library-pool memory.
template <typename Launch>
int colour_helper(const void *in, int64_t npix, size_t in_px, void *out, size_t out_px, int32_t mem_kind, void *hip_stream,
                  Launch launch)
{
    t_err.clear();
    if (npix < 0) return fail(TMFWM_ERR_INVALID, "npix < 0");
    if (npix == 0) return 0;
    if (int rc = need_device()) return rc;
    hipStream_t st = pick_stream(hip_stream);
    if (mem_kind == TMFWM_MEM_DEVICE) {
        if (int rc = check_device_ptr(in, "input")) return rc;
        if (int rc = check_device_ptr(out, "output")) return rc;
        TMF_HIP(launch(in, out, st));
        return 0;
    }
    if (mem_kind != TMFWM_MEM_HOST || !in || !out) return fail(TMFWM_ERR_INVALID, "bad host arguments");
    DevBuf di, dout;
    if (int rc = di.alloc((size_t)npix * in_px, st, "input pixels")) return rc;
    if (int rc = dout.alloc((size_t)npix * out_px, st, "output pixels")) return rc;
    TMF_HIP(hipMemcpyAsync(di.p, in, (size_t)npix * in_px, hipMemcpyHostToDevice, st));
    TMF_HIP(launch(di.p, dout.p, st));
    TMF_HIP(hipMemcpyAsync(out, dout.p, (size_t)npix * out_px, hipMemcpyDeviceToHost, st));
    TMF_HIP(hipStreamSynchronize(st));
    return 0;
}

size_t dtype_bytes(int32_t dtype)
{
    switch (dtype) {
    case TMFWM_DT_F16: return 2;
    case TMFWM_DT_F32: return 4;
    case TMFWM_DT_F64: return 8;
    default: return 0;
    }
}

}  // namespace
}  // extern "C++"

int tmfwm_rgb_to_ycbcr(const uint8_t *rgb, int64_t npix, float *ycc, int32_t mem_kind, void *hip_stream)
{
    return colour_helper(rgb, npix, 3, ycc, 12, mem_kind, hip_stream, [npix](const void *i, void *o, hipStream_t st) {
        return tmf::launch_rgb_to_ycbcr(static_cast<const uint8_t *>(i), npix, static_cast<float *>(o), st);
    });
}

int tmfwm_rgb_to_ycbcr_f32(const float *rgb, int64_t npix, float *ycc, int32_t mem_kind, void *hip_stream)
{
    return colour_helper(rgb, npix, 12, ycc, 12, mem_kind, hip_stream, [npix](const void *i, void *o, hipStream_t st) {
        return tmf::launch_rgb_to_ycbcr_f32(static_cast<const float *>(i), npix, static_cast<float *>(o), st);
    });
}

int tmfwm_ycbcr_to_rgb_typed(const void *ycc, int32_t dtype, int64_t npix, uint8_t *rgb, int32_t mem_kind, void *hip_stream)
{
    const size_t eb = dtype_bytes(dtype);
    if (!eb) {
        t_err.clear();
        return fail(TMFWM_ERR_INVALID, "dtype %d (TMFWM_DT_F16 / _F32 / _F64)", dtype);
    }
    return colour_helper(ycc, npix, 3 * eb, rgb, 3, mem_kind, hip_stream, [npix, dtype](const void *i, void *o, hipStream_t st) {
        return tmf::launch_ycbcr_to_rgb(i, dtype, npix, static_cast<uint8_t *>(o), st);
    });
}

int tmfwm_ycbcr_to_rgb(const float *ycc, int64_t npix, uint8_t *rgb, int32_t mem_kind, void *hip_stream)
{
    return tmfwm_ycbcr_to_rgb_typed(ycc, TMFWM_DT_F32, npix, rgb, mem_kind, hip_stream);
}

int tmfwm_dct2d_blocks(float *blocks, int64_t n_blocks, int32_t block, int32_t inverse, int32_t mem_kind, void *hip_stream)
{
    t_err.clear();
    if (n_blocks < 0) return fail(TMFWM_ERR_INVALID, "n_blocks < 0");
    if (int rc = check_frames(0, 0, 0, 0, block)) return rc;
    if (int rc = need_device()) return rc;
    if (n_blocks == 0) return 0;
    hipStream_t st = pick_stream(hip_stream);
    const size_t bytes = (size_t)n_blocks * block * block * sizeof(float);
    if (mem_kind == TMFWM_MEM_DEVICE) {
        if (int rc = check_device_ptr(blocks, "blocks")) return rc;
        TMF_HIP(tmf::launch_dct2d_blocks(blocks, n_blocks, block, inverse != 0, st));
        return 0;
    }
    if (mem_kind != TMFWM_MEM_HOST || !blocks) return fail(TMFWM_ERR_INVALID, "bad host arguments");
    DevBuf d;
    if (int rc = d.alloc(bytes, st, "blocks")) return rc;
    TMF_HIP(hipMemcpyAsync(d.p, blocks, bytes, hipMemcpyHostToDevice, st));
    TMF_HIP(tmf::launch_dct2d_blocks(static_cast<float *>(d.p), n_blocks, block, inverse != 0, st));
    TMF_HIP(hipMemcpyAsync(blocks, d.p, bytes, hipMemcpyDeviceToHost, st));
    TMF_HIP(hipStreamSynchronize(st));
    return 0;
}

int tmfwm_svd_blocks(const float *D, int64_t n_blocks, int32_t block, float *U, float *S, float *Vt, int32_t *sweeps,
                     int32_t mem_kind, void *hip_stream)
{
    t_err.clear();
    if (n_blocks < 0) return fail(TMFWM_ERR_INVALID, "n_blocks < 0");
    if (int rc = check_frames(0, 0, 0, 0, block)) return rc;
    if (int rc = need_device()) return rc;
    if (n_blocks == 0) return 0;
    hipStream_t st = pick_stream(hip_stream);
    const size_t mb = (size_t)n_blocks * block * block * sizeof(float), sb = (size_t)n_blocks * block * sizeof(float);
    if (mem_kind == TMFWM_MEM_DEVICE) {
        for (auto [p, nm] : {std::pair<const void *, const char *>{D, "D"}, {U, "U"}, {S, "S"}, {Vt, "Vt"}})
            if (int rc = check_device_ptr(p, nm)) return rc;
        if (sweeps)
            if (int rc = check_device_ptr(sweeps, "sweeps")) return rc;
        TMF_HIP(tmf::launch_svd_blocks(D, n_blocks, block, U, S, Vt, sweeps, st));
        return 0;
    }
    if (mem_kind != TMFWM_MEM_HOST || !D || !U || !S || !Vt) return fail(TMFWM_ERR_INVALID, "bad host arguments");
    DevBuf dD, dU, dS, dV, dW;
    if (int rc = dD.alloc(mb, st, "D")) return rc;
    if (int rc = dU.alloc(mb, st, "U")) return rc;
    if (int rc = dS.alloc(sb, st, "S")) return rc;
    if (int rc = dV.alloc(mb, st, "Vt")) return rc;
    if (sweeps)
        if (int rc = dW.alloc((size_t)n_blocks * 4, st, "sweeps")) return rc;
    TMF_HIP(hipMemcpyAsync(dD.p, D, mb, hipMemcpyHostToDevice, st));
    TMF_HIP(tmf::launch_svd_blocks(static_cast<const float *>(dD.p), n_blocks, block, static_cast<float *>(dU.p),
                                   static_cast<float *>(dS.p), static_cast<float *>(dV.p), static_cast<int32_t *>(dW.p), st));
    TMF_HIP(hipMemcpyAsync(U, dU.p, mb, hipMemcpyDeviceToHost, st));
    TMF_HIP(hipMemcpyAsync(S, dS.p, sb, hipMemcpyDeviceToHost, st));
    TMF_HIP(hipMemcpyAsync(Vt, dV.p, mb, hipMemcpyDeviceToHost, st));
    if (sweeps) TMF_HIP(hipMemcpyAsync(sweeps, dW.p, (size_t)n_blocks * 4, hipMemcpyDeviceToHost, st));
    TMF_HIP(hipStreamSynchronize(st));
    return 0;
}

int tmfwm_lapack_svd_blocks(const float *D, int64_t n_blocks, int32_t block, float *U, float *S, float *Vt, int32_t want_vectors,
                            int32_t mem_kind, void *hip_stream)
{
    t_err.clear();
    if (n_blocks < 0) return fail(TMFWM_ERR_INVALID, "n_blocks < 0");
    if (int rc = check_frames(0, 0, 0, 0, block)) return rc;
    if (int rc = need_device()) return rc;
    if (n_blocks == 0) return 0;
    hipStream_t st = pick_stream(hip_stream);
    const size_t mb = (size_t)n_blocks * block * block * sizeof(float), sb = (size_t)n_blocks * block * sizeof(float);
    DevBuf dinfo;
    if (int rc = dinfo.alloc((size_t)n_blocks * 4, st, "info")) return rc;
    int32_t *info = static_cast<int32_t *>(dinfo.p);
    const float *dD = D;
    float *dU = U, *dS = S, *dVt = Vt;
    DevBuf bD, bU, bS, bV;
    if (mem_kind == TMFWM_MEM_DEVICE) {
        if (int rc = check_device_ptr(D, "D")) return rc;
        if (int rc = check_device_ptr(S, "S")) return rc;
        if (want_vectors) {
            if (int rc = check_device_ptr(U, "U")) return rc;
            if (int rc = check_device_ptr(Vt, "Vt")) return rc;
        }
    } else {
        if (mem_kind != TMFWM_MEM_HOST || !D || !S || (want_vectors && (!U || !Vt))) return fail(TMFWM_ERR_INVALID, "bad host arguments");
        if (int rc = bD.alloc(mb, st, "D")) return rc;
        if (int rc = bS.alloc(sb, st, "S")) return rc;
        if (want_vectors) {
            if (int rc = bU.alloc(mb, st, "U")) return rc;
            if (int rc = bV.alloc(mb, st, "Vt")) return rc;
        }
        TMF_HIP(hipMemcpyAsync(bD.p, D, mb, hipMemcpyHostToDevice, st));
        dD = static_cast<const float *>(bD.p);
        dS = static_cast<float *>(bS.p);
        dU = static_cast<float *>(bU.p);
        dVt = static_cast<float *>(bV.p);
    }
    TMF_HIP(tmf::launch_lapack_svd_blocks(dD, n_blocks, block, dU, dS, dVt, want_vectors != 0, info, st));
    if (mem_kind == TMFWM_MEM_HOST) {
        TMF_HIP(hipMemcpyAsync(S, dS, sb, hipMemcpyDeviceToHost, st));
        if (want_vectors) {
            TMF_HIP(hipMemcpyAsync(U, dU, mb, hipMemcpyDeviceToHost, st));
            TMF_HIP(hipMemcpyAsync(Vt, dVt, mb, hipMemcpyDeviceToHost, st));
        }
    }
    // dbdsqr's convergence flag of every block (LAPACK's info > 0): reported, never silent
    std::vector<int32_t> h((size_t)n_blocks);
    TMF_HIP(hipMemcpyAsync(h.data(), info, (size_t)n_blocks * 4, hipMemcpyDeviceToHost, st));
    TMF_HIP(hipStreamSynchronize(st));
    for (int64_t k = 0; k < n_blocks; ++k)
        if (h[(size_t)k]) return fail(TMFWM_ERR_INVALID, "dbdsqr did not converge on block %lld", (long long)k);
    return 0;
}

int tmfwm_lapack_nrm2(const double *x, int64_t n_vectors, int32_t n, int32_t inc, double *out, int32_t mem_kind, void *hip_stream)
{
    t_err.clear();
    if (n_vectors < 0 || n < 0 || inc < 1) return fail(TMFWM_ERR_INVALID, "bad sizes");
    if (int rc = need_device()) return rc;
    if (n_vectors == 0) return 0;
    hipStream_t st = pick_stream(hip_stream);
    const size_t xb = (size_t)n_vectors * n * inc * sizeof(double), ob = (size_t)n_vectors * sizeof(double);
    if (mem_kind == TMFWM_MEM_DEVICE) {
        if (xb)
            if (int rc = check_device_ptr(x, "x")) return rc;
        if (int rc = check_device_ptr(out, "out")) return rc;
        TMF_HIP(tmf::launch_lapack_nrm2(x, n_vectors, n, inc, out, st));
        return 0;
    }
    if (mem_kind != TMFWM_MEM_HOST || !out || (xb && !x)) return fail(TMFWM_ERR_INVALID, "bad host arguments");
    DevBuf dx, dout;
    if (int rc = dx.alloc(xb, st, "x")) return rc;
    if (int rc = dout.alloc(ob, st, "out")) return rc;
    if (xb) TMF_HIP(hipMemcpyAsync(dx.p, x, xb, hipMemcpyHostToDevice, st));
    TMF_HIP(tmf::launch_lapack_nrm2(static_cast<const double *>(dx.p), n_vectors, n, inc, static_cast<double *>(dout.p), st));
    TMF_HIP(hipMemcpyAsync(out, dout.p, ob, hipMemcpyDeviceToHost, st));
    TMF_HIP(hipStreamSynchronize(st));
    return 0;
}

int tmfwm_synth_frames(uint64_t seed, int64_t frame0, int64_t n_frames, int64_t frame_bytes, uint8_t *out, void *hip_stream)
{
    t_err.clear();
    if (n_frames < 0 || frame_bytes < 0 || frame0 < 0) return fail(TMFWM_ERR_INVALID, "negative size");
    if (n_frames == 0 || frame_bytes == 0) return 0;
    if (int rc = need_device()) return rc;
    if (int rc = check_device_ptr(out, "out")) return rc;
    TMF_HIP(tmf::launch_synth(seed, frame0, n_frames, frame_bytes, out, pick_stream(hip_stream)));
    return 0;
}

int tmfwm_prepare_tiles(const uint8_t *wm, int64_t n_wm, int32_t wm_height, int32_t wm_width, int64_t wm_stride,
                        int32_t tile_height, int32_t tile_width, int32_t preserve_ratio, uint8_t *tiles, int64_t tile_stride,
                        int32_t mem_kind, void *hip_stream)
{
    t_err.clear();
    if (n_wm < 0) return fail(TMFWM_ERR_INVALID, "n_wm < 0");
    if (wm_height <= 0 || wm_width <= 0 || tile_height <= 0 || tile_width <= 0)
        return fail(TMFWM_ERR_INVALID, "height and width must be > 0 (watermark %dx%d, tile %dx%d)", wm_width, wm_height,
                    tile_width, tile_height);
    const size_t wbytes = (size_t)wm_height * wm_width, tbytes = (size_t)tile_height * tile_width;
    if (wm_stride < (int64_t)wbytes) return fail(TMFWM_ERR_INVALID, "wm_stride %lld < wm_height*wm_width", (long long)wm_stride);
    if (tile_stride < (int64_t)tbytes)
        return fail(TMFWM_ERR_INVALID, "tile_stride %lld < tile_height*tile_width", (long long)tile_stride);
    if (mem_kind != TMFWM_MEM_HOST && mem_kind != TMFWM_MEM_DEVICE) return fail(TMFWM_ERR_INVALID, "mem_kind %d", mem_kind);
    // watermarking.py:105-110: ratio = min(tw/ow, th/oh); new size int(size * ratio)
    int rh = tile_height, rw = tile_width, px = 0, py = 0;
    if (preserve_ratio) {
        const double fw = (double)tile_width / (double)wm_width, fh = (double)tile_height / (double)wm_height;
        const double ratio = fh < fw ? fh : fw;  // Python min() keeps the first of equals
        rw = (int)((double)wm_width * ratio);
        rh = (int)((double)wm_height * ratio);
        if (rw <= 0 || rh <= 0) return fail(TMFWM_ERR_INVALID, "height and width must be > 0 (resized %dx%d)", rw, rh);
        px = (tile_width - rw) / 2;  // :120-121
        py = (tile_height - rh) / 2;
    }
    const size_t wspan = span_bytes(n_wm, wm_stride, (int64_t)wbytes), tspan = span_bytes(n_wm, tile_stride, (int64_t)tbytes);
    if (n_wm > 0) {
        if (mem_kind == TMFWM_MEM_DEVICE) {
            if (int rc = check_device_ptr(wm, "wm")) return rc;
            if (int rc = check_device_ptr(tiles, "tiles")) return rc;
            if (ranges_overlap(wm, wspan, tiles, tspan)) return fail(TMFWM_ERR_INVALID, "tiles overlaps wm");
        } else if (!wm || !tiles) {
            return fail(TMFWM_ERR_INVALID, "NULL host pointer");
        }
    }
    if (int rc = need_device()) return rc;
    if (n_wm == 0) return 0;
    hipStream_t st = pick_stream(hip_stream);
    tmf::ResamplePlan plan;
    plan.build(wm_height, wm_width, rh, rw);
    const std::vector<int> tables = plan.pack();  // one plan, one upload for the whole batch
    DevBuf dtab, dtmp, dwm, dtile;
    if (int rc = dtab.alloc(tables.size() * sizeof(int), st, "resample tables")) return rc;
    if (int rc = dtmp.alloc(tmf::resize_tmp_bytes(plan, n_wm), st, "resample scratch")) return rc;
    const uint8_t *src = wm;
    uint8_t *dst = tiles;
    int64_t sstride = wm_stride, dstride = tile_stride;
    if (mem_kind == TMFWM_MEM_HOST) {  // staged compact: the caller's bytes between watermarks / tiles are not touched
        sstride = (int64_t)wbytes;
        dstride = (int64_t)tbytes;
        if (int rc = dwm.alloc(wbytes * (size_t)n_wm, st, "watermarks")) return rc;
        if (int rc = dtile.alloc(tbytes * (size_t)n_wm, st, "tiles")) return rc;
        if (int rc = copy_items(dwm.p, wm, wbytes, n_wm, wm_stride, hipMemcpyHostToDevice, st)) return rc;
        src = static_cast<const uint8_t *>(dwm.p);
        dst = static_cast<uint8_t *>(dtile.p);
    }
    TMF_HIP(hipMemcpyAsync(dtab.p, tables.data(), tables.size() * sizeof(int), hipMemcpyHostToDevice, st));
    if (preserve_ratio) {  // Image.new("L", ..., 255) (:116)
        if (n_wm == 1 || dstride == (int64_t)tbytes)
            TMF_HIP(hipMemsetAsync(dst, 255, tbytes * (size_t)n_wm, st));
        else
            TMF_HIP(hipMemset2DAsync(dst, (size_t)dstride, 255, tbytes, (size_t)n_wm, st));
    }
    TMF_HIP(tmf::launch_resize_lanczos_batch(src, sstride, n_wm, plan, static_cast<const int *>(dtab.p),
                                             static_cast<uint8_t *>(dtmp.p), dst + (size_t)py * tile_width + px, tile_width, dstride,
                                             st));
    if (mem_kind == TMFWM_MEM_HOST) {
        if (int rc = copy_items(dst, tiles, tbytes, n_wm, tile_stride, hipMemcpyDeviceToHost, st)) return rc;
    }
    // the host-side tables (and, for the host path, the result) must outlive the copies
    TMF_HIP(hipStreamSynchronize(st));
    return 0;
}

int tmfwm_prepare_tile(const uint8_t *wm, int32_t wm_height, int32_t wm_width, int32_t tile_height, int32_t tile_width,
                       int32_t preserve_ratio, uint8_t *tile, int32_t mem_kind, void *hip_stream)
{
    // the batched call with one watermark (the size check comes before the stride checks)
    return tmfwm_prepare_tiles(wm, 1, wm_height, wm_width, (int64_t)wm_height * wm_width, tile_height, tile_width, preserve_ratio,
                               tile, (int64_t)tile_height * tile_width, mem_kind, hip_stream);
}

// ---- ragged batches (tmfwm_ragged.h): frames of mixed sizes through one set of launches
extern "C++" {
namespace {

// What a ragged call does with its frames.  The kind decides each piece's byte count, which
// pieces are inputs, whether an edge pass runs and which launchers run.
enum class RKind {
    Embed,    // in0 = rgb, in1 = wm_tile (bytes), out = the output pixels
    Extract,  // in0 = wm_rgb, in1 = orig_rgb, out = out_tile (bytes)
    Map,      // in0 = rgb, no in1, out = out_key (floats)
    Keyed,    // in0 = wm_rgb, in1 = key (floats), out = out_tile (bytes)
    EmbedKey, // Embed, and out2 = out_key (floats): the frame's second output
};
bool embeds(RKind k) { return k == RKind::Embed || k == RKind::EmbedKey; }

// One frame of a ragged call once its descriptor is checked; the descriptor array is not read
// after that.
struct RFrame {
    const uint8_t *in0, *in1;
    uint8_t *out;
    int32_t H, W;
    uint8_t *out2 = nullptr;  // RKind::EmbedKey only
    int32_t px = 3;           // bytes per pixel of in0 (4: the keyed *_ragged_px calls, one layout per call)
    double alpha = 0.0;       // the *_ragged_alphas calls: the frame's own alpha
    int64_t pixel_bytes() const { return (int64_t)H * W * px; }
    int64_t tile_bytes(int b) const { return (int64_t)(H / b) * (W / b); }
    // the bytes behind in1 and out
    int64_t in1_bytes(RKind k, int b) const
    {
        return embeds(k) ? tile_bytes(b) : k == RKind::Extract ? pixel_bytes() : k == RKind::Keyed ? tile_bytes(b) * 4 : 0;
    }
    int64_t out_bytes(RKind k, int b) const
    {
        return embeds(k) ? pixel_bytes() : k == RKind::Map ? tile_bytes(b) * 4 : tile_bytes(b);
    }
    int64_t out2_bytes(RKind k, int b) const { return k == RKind::EmbedKey ? tile_bytes(b) * 4 : 0; }
    // embed writes every frame that has a pixel (its colour round trip); the others only frames with a block
    bool has_work(RKind k, int b) const { return pixel_bytes() > 0 && (embeds(k) || tile_bytes(b) > 0); }
};

const char *const kRaggedNames[5][3] = {{"rgb", "wm_tile", "out"}, {"wm_rgb", "orig_rgb", "out_tile"}, {"rgb", "", "out_key"},
                                        {"wm_rgb", "key", "out_tile"}, {"rgb", "wm_tile", "out"}};

// the checks every ragged call makes before it touches the device
int check_ragged_call(const void *frames, int64_t n, int32_t block, double alpha, RKind kind, int32_t mem_kind, int32_t route,
                      int64_t *n_lapack, bool rank1_routes = false)
{
    const bool extract = kind == RKind::Extract || kind == RKind::Keyed;
    // the rank-1 routes: tmfwm_embed_ragged_rank1 / tmfwm_embed_key_ragged_rank1 alone (the one ragged list pass)
    if (int rc = begin_call(route, n_lapack, rank1_routes)) return rc;
    if (n < 0) return fail(TMFWM_ERR_INVALID, "negative size (n=%lld)", (long long)n);
    if (n > 0 && !frames) return fail(TMFWM_ERR_INVALID, "frames is NULL");
    if (!supported_block(block)) return fail(TMFWM_ERR_UNSUPPORTED, "block size %d not supported (even, 4..16)", block);
    if (mem_kind != TMFWM_MEM_HOST && mem_kind != TMFWM_MEM_DEVICE) return fail(TMFWM_ERR_INVALID, "mem_kind %d", mem_kind);
    if (kind != RKind::Map && (extract ? (!std::isfinite(alpha) || alpha == 0.0) : !std::isfinite(alpha)))  // the map takes no alpha
        return fail(TMFWM_ERR_INVALID, extract ? "alpha must be finite and non-zero" : "alpha is not finite");
    return 0;
}

// the *_ragged_alphas calls: n doubles in host memory, every one checked whether or not its frame has a block
int check_ragged_alphas(const double *alphas, int64_t n, RKind kind)
{
    const bool extract = kind == RKind::Extract || kind == RKind::Keyed;
    if (n > 0 && !alphas) return fail(TMFWM_ERR_INVALID, "alphas is NULL");
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(alphas[i]) || (extract && alphas[i] == 0.0))
            return fail(TMFWM_ERR_INVALID, extract ? "frame %lld: alpha must be finite and non-zero" : "frame %lld: alpha is not finite",
                        (long long)i);
    return 0;
}

// one frame's sizes and pointers (the tile and key pointers only where the frame has a block)
int check_ragged_frame(int64_t i, const RFrame &f, int32_t block, RKind kind)
{
    if (int rc = check_frames(1, f.H, f.W, (int64_t)f.H * f.W * 3, block)) return fail(rc, "frame %lld: %s", (long long)i, t_err.c_str());
    if (f.H == 0 || f.W == 0) return 0;
    if (f.tile_bytes(block) > 0x7FFFFFFFll) return fail(TMFWM_ERR_INVALID, "frame %lld: more than 2^31 - 1 blocks", (long long)i);
    const bool tile = f.tile_bytes(block) > 0;
    if (embeds(kind) ? (!f.in0 || !f.out || (tile && (!f.in1 || (kind == RKind::EmbedKey && !f.out2))))
                     : (tile && (!f.in0 || (kind != RKind::Map && !f.in1) || !f.out)))
        return fail(TMFWM_ERR_INVALID, "frame %lld: NULL pointer in the descriptor", (long long)i);
    // the float pieces are read and written as floats
    const uint8_t *fl = kind == RKind::Keyed ? f.in1 : kind == RKind::Map ? f.out : kind == RKind::EmbedKey ? f.out2 : nullptr;
    if (tile && reinterpret_cast<uintptr_t>(fl) % 4)
        return fail(TMFWM_ERR_INVALID, "frame %lld: %s is not 4-byte aligned", (long long)i,
                    kind == RKind::EmbedKey ? "out_key" : kRaggedNames[(int)kind][kind == RKind::Keyed ? 1 : 2]);
    return 0;
}

// No output of the call may share a byte with an input or with another output: the intervals
// sorted by start, one sweep that keeps the furthest end of the inputs and of the outputs so far.
struct Span {
    uintptr_t lo, hi;
    bool out;
    int64_t frame;
};

int check_ragged_overlap(std::vector<Span> &spans, const char *unit = "frame")  // unit: what Span::frame counts
{
    std::sort(spans.begin(), spans.end(), [](const Span &a, const Span &b) { return a.lo < b.lo; });
    uintptr_t in_hi = 0, out_hi = 0;
    int64_t in_f = -1, out_f = -1;
    for (const Span &s : spans) {
        if (s.lo == s.hi) continue;
        if (s.out && s.lo < in_hi) return fail(TMFWM_ERR_INVALID, "%s %lld's output overlaps an input of %s %lld", unit, (long long)s.frame, unit, (long long)in_f);
        if (s.out && s.lo < out_hi) return fail(TMFWM_ERR_INVALID, "%s %lld's output overlaps %s %lld's", unit, (long long)s.frame, unit, (long long)out_f);
        if (!s.out && s.lo < out_hi) return fail(TMFWM_ERR_INVALID, "%s %lld's output overlaps an input of %s %lld", unit, (long long)out_f, unit, (long long)s.frame);
        if (s.out && s.hi > out_hi) out_hi = s.hi, out_f = s.frame;
        if (!s.out && s.hi > in_hi) in_hi = s.hi, in_f = s.frame;
    }
    return 0;
}

int check_ragged_device(const std::vector<RFrame> &fr, int32_t block, RKind kind)
{
    const char *const *name = kRaggedNames[(int)kind];
    std::vector<Span> spans;
    spans.reserve(fr.size() * 3);
    auto add = [&](const void *p, int64_t bytes, bool out, int64_t i) {
        const uintptr_t lo = reinterpret_cast<uintptr_t>(p);
        spans.push_back({lo, lo + (uintptr_t)bytes, out, i});
    };
    for (size_t i = 0; i < fr.size(); ++i) {
        const RFrame &f = fr[i];
        const int64_t ib = f.in1_bytes(kind, block), kb = f.out2_bytes(kind, block);
        if (!f.has_work(kind, block)) continue;
        if (int rc = check_device_ptr(f.in0, name[0])) return rc;
        if (ib)
            if (int rc = check_device_ptr(f.in1, name[1])) return rc;
        if (int rc = check_device_ptr(f.out, name[2])) return rc;
        if (kb)
            if (int rc = check_device_ptr(f.out2, "out_key")) return rc;
        add(f.in0, f.pixel_bytes(), false, (int64_t)i);
        if (ib) add(f.in1, ib, false, (int64_t)i);
        add(f.out, f.out_bytes(kind, block), true, (int64_t)i);
        if (kb) add(f.out2, kb, true, (int64_t)i);
    }
    return check_ragged_overlap(spans);
}

// Pinned host buffers for the frame table of an asynchronous call: the table is built in one,
// copied to the device on the call's stream, and the buffer goes back to the free list with an
// event recorded behind the copy; whoever takes it next waits for that event first.
struct TableSlot {
    void *p = nullptr;
    size_t cap = 0;
    int dev = 0;
    hipEvent_t ev = nullptr;
};
std::mutex g_table_mu;
std::vector<TableSlot> g_tables;
constexpr size_t kTableSlots = 8;

void drop_table(TableSlot &s)
{
    if (s.ev) {
        (void)hipEventSynchronize(s.ev);
        (void)hipEventDestroy(s.ev);
    }
    if (s.p) (void)hipHostFree(s.p);
    (void)hipGetLastError();
    s = TableSlot{};
}

int take_table(size_t bytes, int dev, TableSlot &s)
{
    {
        std::lock_guard<std::mutex> g(g_table_mu);
        for (size_t i = 0; i < g_tables.size(); ++i)
            if (g_tables[i].dev == dev && g_tables[i].cap >= bytes) {
                s = g_tables[i];
                g_tables.erase(g_tables.begin() + (long)i);
                break;
            }
    }
    if (s.p) {
        TMF_HIP(hipEventSynchronize(s.ev));  // the last copy out of it is done
        return 0;
    }
    s.dev = dev;
    s.cap = bytes < 16384 ? 16384 : bytes;
    if (hipHostMalloc(&s.p, s.cap, hipHostMallocDefault) != hipSuccess ||
        hipEventCreateWithFlags(&s.ev, hipEventDisableTiming) != hipSuccess) {
        drop_table(s);
        return fail(TMFWM_ERR_NOMEM, "pinned allocation of %zu bytes for the frame table failed", bytes);
    }
    return 0;
}

void give_table(TableSlot &s, hipStream_t st)
{
    if (!s.p) return;
    if (hipEventRecord(s.ev, st) != hipSuccess) {  // cannot tell when the copy ends: wait for it
        (void)hipGetLastError();
        (void)hipStreamSynchronize(st);
    }
    std::lock_guard<std::mutex> g(g_table_mu);
    if (g_tables.size() < kTableSlots) g_tables.push_back(s);
    else drop_table(s);
    s = TableSlot{};
}

// Chunks of whole frames: at most list_cap() blocks each (block ids are 32-bit and relative to
// the chunk; a frame that alone has more is a chunk of its own, as Chunks::plan has it) and few
// enough edge pixels for one launch of the edge pass.
struct RaggedChunk {
    int64_t first = 0, n = 0, waves = 0, blocks = 0, edge = 0;
    int64_t with_blocks = 0;  // frames that have a block
    uint32_t shards = 0;      // TMFWM_ROUTE_RANK1: the list-pass shards the chunk uses
};
constexpr int64_t kEdgeCap = int64_t(1) << 38;

bool rank1_route(int route) { return route == TMFWM_ROUTE_RANK1 || route == TMFWM_ROUTE_RANK1_REFERENCE; }

// What run_ragged takes: the frame table of the frames that have work, with chunk-relative
// prefixes, the chunks, and the table's side tables -- RKind::EmbedKey: each entry's key output;
// TMFWM_ROUTE_RANK1: each entry's list-pass shards, relative to its chunk as the ids are; the
// *_ragged_alphas calls: each entry's alpha.
struct RaggedPlan {
    RKind kind;
    int route;
    std::vector<tmf::RaggedFrame> table;
    std::vector<RaggedChunk> chunks;
    std::vector<float *> keys;
    std::vector<tmf::RaggedShards> shards;
    std::vector<tmf::RaggedAlpha> alphas;
};

void plan_ragged(const std::vector<RFrame> &fr, int32_t block, RKind kind, int route, RaggedPlan &plan, bool per_frame = false)
{
    plan.kind = kind;
    plan.route = route;
    std::vector<tmf::RaggedFrame> &table = plan.table;
    std::vector<RaggedChunk> &chunks = plan.chunks;
    std::vector<float *> &keys = plan.keys;
    const bool list_pass = route == TMFWM_ROUTE_RANK1;
    const int bpw = tmf::ragged_strip_blocks(block);
    const int64_t cap = list_cap();
    RaggedChunk c;
    for (const RFrame &f : fr) {
        tmf::RaggedFrame t{};
        t.in0 = f.in0;
        t.in1 = f.in1;
        t.out = f.out;
        t.H = f.H;
        t.W = f.W;
        t.nbh = f.H / block;
        t.nbw = f.W / block;
        t.strips_per_row = (t.nbw + bpw - 1) / bpw;
        // the frame's pixel buffers: two of them, or the single one of the keyed calls
        t.aligned = f.px == 4 ? (int32_t)tmf::keyed_aligned(f.in0, 0, f.W, 4)
                              : (int32_t)tmf::dev_aligned(f.in0, embeds(kind) ? f.out : kind == RKind::Extract ? f.in1 : f.in0, 0, f.W);
        const int64_t waves = (int64_t)t.nbh * t.strips_per_row, blocks = (int64_t)t.nbh * t.nbw;
        const int64_t edge = embeds(kind) ? (int64_t)f.H * f.W - blocks * block * block : 0;
        if (blocks == 0 && edge == 0) continue;
        if (c.n > 0 && (c.blocks + blocks > cap || c.edge + edge > kEdgeCap ||
                        (list_pass && blocks > 0 && tmf::ragged_shards_full(c.with_blocks)))) {
            chunks.push_back(c);
            c = RaggedChunk{};
            c.first = (int64_t)table.size();
        }
        t.wave0 = (uint32_t)c.waves;
        t.block0 = (uint32_t)c.blocks;
        t.edge0 = c.edge;
        table.push_back(t);
        if (kind == RKind::EmbedKey) keys.push_back(reinterpret_cast<float *>(f.out2));
        if (per_frame) plan.alphas.push_back(tmf::RaggedAlpha{f.alpha, (float)f.alpha, 0.0f});
        ++c.n;
        c.with_blocks += blocks > 0;
        c.waves += waves;
        c.blocks += blocks;
        c.edge += edge;
    }
    if (c.n > 0) chunks.push_back(c);
    if (list_pass) {
        plan.shards.resize(table.size());
        for (RaggedChunk &k : chunks) k.shards = tmf::ragged_plan_shards(table.data() + k.first, k.n, plan.shards.data() + k.first);
    }
}

size_t round16(size_t n) { return (n + 15) & ~size_t(15); }

// Both passes of a ragged call over device-resident frames: the frame table uploaded, then the
// chunks through two_pass, with the edge pass between a chunk's first pass and its fixup pass and
// neither of the two for a chunk without a block.  (alpha: the uniform calls'; a plan with an
// alpha table runs the per-frame kernels, which do not read it)
int run_ragged(int32_t block, double alpha, hipStream_t st, const Report &rep, const RaggedPlan &plan,
               int px = 3)  // px: the keyed kinds' bytes per pixel
{
    const RKind kind = plan.kind;
    const int route = plan.route;
    const std::vector<tmf::RaggedFrame> &table = plan.table;
    const std::vector<RaggedChunk> &chunks = plan.chunks;
    const std::vector<float *> &keys = plan.keys;
    if (chunks.empty()) return 0;
    // on a rank-1 route the strip launch is the pre-pass (the plain embed alone: the key call composes, ragged_call)
    const bool pre = rank1_route(route) && kind == RKind::Embed && tmf::rank1_block(block);
    const bool list_pass = pre && route == TMFWM_ROUTE_RANK1;
    // the frame table and behind it the side tables -- the keys (RKind::EmbedKey), the list-pass
    // shards (TMFWM_ROUTE_RANK1), the alphas (the *_ragged_alphas calls); empty otherwise -- in one upload
    const size_t fbytes = table.size() * sizeof(tmf::RaggedFrame), kbytes = keys.size() * sizeof(float *);
    const size_t sbytes = plan.shards.size() * sizeof(tmf::RaggedShards);
    const size_t abase = round16(fbytes + kbytes + sbytes);  // (a chunk's kernels find its entries by their distance from its frames)
    const size_t tbytes = abase + plan.alphas.size() * sizeof(tmf::RaggedAlpha);
    if (tbytes > 0xFFFFFFFFull) return fail(TMFWM_ERR_INVALID, "too many frames for one call (%zu)", table.size());
    TableSlot slot;
    if (int rc = take_table(tbytes, stream_device(st), slot)) return rc;
    std::copy(table.begin(), table.end(), static_cast<tmf::RaggedFrame *>(slot.p));
    std::copy(keys.begin(), keys.end(), reinterpret_cast<float **>(static_cast<uint8_t *>(slot.p) + fbytes));
    std::copy(plan.shards.begin(), plan.shards.end(), reinterpret_cast<tmf::RaggedShards *>(static_cast<uint8_t *>(slot.p) + fbytes + kbytes));
    std::copy(plan.alphas.begin(), plan.alphas.end(),
              reinterpret_cast<tmf::RaggedAlpha *>(static_cast<uint8_t *>(slot.p) + abase));
    DevBuf dtable;
    int rc = dtable.alloc(tbytes, st, "frame table");
    if (rc == 0 && hipMemcpyAsync(dtable.p, slot.p, tbytes, hipMemcpyHostToDevice, st) != hipSuccess)
        rc = fail(TMFWM_ERR_HIP, "copying the frame table failed: %s", hipGetErrorString(hipGetLastError()));
    give_table(slot, st);
    if (rc) return rc;
    std::vector<int64_t> blocks;
    for (const RaggedChunk &k : chunks) blocks.push_back(k.blocks);
    // a chunk's slice of the alpha table, as its slice of the frame table: entry k.first, seen from frame k.first
    auto alphas_off = [&](const RaggedChunk &k) -> uint32_t {
        return plan.alphas.empty() ? 0u : (uint32_t)(abase + (size_t)k.first * sizeof(tmf::RaggedAlpha) - (size_t)k.first * sizeof(tmf::RaggedFrame));
    };
    return two_pass(blocks, list_pass, true, st, rep, [&](int64_t c, const ChunkLists &w) -> int {
        const RaggedChunk &k = chunks[(size_t)c];
        if (pre) {  // the pre-pass (+ its list pass on TMFWM_ROUTE_RANK1), the edges, the dgesdd route
            tmf::RaggedRank1Args r{};
            r.frames = static_cast<const tmf::RaggedFrame *>(dtable.p) + k.first;
            r.nframes = (int32_t)k.n;
            r.block = block;
            r.alpha = alpha;
            r.alpha32 = (float)alpha;
            r.alphas_off = alphas_off(k);
            r.fb_list = w.fb_list;
            r.fb_count = w.fb_count;
            r.fb_bad = w.fb_bad;
            if (list_pass) {  // ids and shard ranges are relative to the chunk
                r.shards = reinterpret_cast<const tmf::RaggedShards *>(static_cast<const uint8_t *>(dtable.p) + fbytes + kbytes) + k.first;
                r.slow_list = w.slow_list;
                r.slow_count = w.slow_count;
                r.slow_shards = w.slow_shards;
            }
            if (k.blocks > 0) TMF_HIP(tmf::launch_embed_rank1_ragged(r, k.waves, k.shards, st));
            TMF_HIP(tmf::launch_edges_ragged(r, k.edge, st));
            if (k.blocks > 0) TMF_HIP(tmf::launch_embed_ragged_fixup(r, r.fb_list, r.fb_count, k.blocks, st));
            return 0;
        }
        tmf::RaggedKeyArgs r{};  // (the other kinds take its RaggedArgs part)
        r.frames = static_cast<const tmf::RaggedFrame *>(dtable.p) + k.first;
        r.nframes = (int32_t)k.n;
        r.block = block;
        r.alpha = alpha;
        r.alpha32 = (float)alpha;
        r.alphas_off = alphas_off(k);
        r.fb_list = w.fb_list;  // no list pass in a ragged call
        r.fb_count = w.fb_count;
        r.fb_bad = w.fb_bad;
        if (kind == RKind::EmbedKey) r.keys = reinterpret_cast<float *const *>(static_cast<const uint8_t *>(dtable.p) + fbytes) + k.first;
        if (k.blocks > 0) {
            if (route == TMFWM_ROUTE_REFERENCE) TMF_HIP(tmf::launch_list_all(r.fb_list, r.fb_count, k.blocks, st));
            else
                TMF_HIP(kind == RKind::EmbedKey  ? tmf::launch_embed_key_ragged(r, k.waves, st)
                        : kind == RKind::Embed   ? tmf::launch_embed_ragged(r, k.waves, st)
                        : kind == RKind::Extract ? tmf::launch_extract_ragged(r, k.waves, st)
                        : kind == RKind::Map     ? tmf::launch_sigma1_map_ragged(r, k.waves, st, px)
                                                 : tmf::launch_extract_keyed_ragged(r, k.waves, st, px));
        }
        if (embeds(kind)) TMF_HIP(tmf::launch_edges_ragged(r, k.edge, st));
        if (k.blocks > 0)
            TMF_HIP(kind == RKind::EmbedKey  ? tmf::launch_embed_key_ragged_fixup(r, r.fb_list, r.fb_count, k.blocks, st)
                    : kind == RKind::Embed   ? tmf::launch_embed_ragged_fixup(r, r.fb_list, r.fb_count, k.blocks, st)
                    : kind == RKind::Extract ? tmf::launch_extract_ragged_fixup(r, r.fb_list, r.fb_count, k.blocks, st)
                    : kind == RKind::Map     ? tmf::launch_sigma1_ragged_fixup(r, r.fb_list, r.fb_count, k.blocks, st, px)
                                             : tmf::launch_extract_keyed_ragged_fixup(r, r.fb_list, r.fb_count, k.blocks, st, px));
        return 0;
    });
}

int ragged_call(std::vector<RFrame> &fr, int32_t block, double alpha, RKind kind, int32_t mem_kind, void *hip_stream, int32_t route,
                int64_t *n_lapack, bool per_frame = false)  // per_frame: RFrame::alpha of each frame instead of `alpha`
{
    for (size_t i = 0; i < fr.size(); ++i)
        if (int rc = check_ragged_frame((int64_t)i, fr[i], block, kind)) return rc;
    if (int rc = need_device()) return rc;
    if (fr.empty()) return 0;
    hipStream_t st = pick_stream(hip_stream);
    const int px = fr[0].px;  // one layout per call
    // The call's parts, each a plan of its own run through run_ragged on the one stream: one, or --
    // the key call on a rank-1 route, composed as tmfwm_embed_key is (embed_key_composed: the
    // pre-pass stores no key) -- the embed's passes and then tmfwm_sigma1_map_ragged's over the
    // same buffers.  The call's counts are the sums over its parts.
    const bool composed = kind == RKind::EmbedKey && tmf::embed_key_composed(block, route, true) && rank1_route(route);
    struct Part {
        RaggedPlan plan;
        int64_t n = 0;
    };
    std::vector<Part> parts(composed ? 2 : 1);
    auto plan_parts = [&](const std::vector<RFrame> &v) {
        if (!composed) return plan_ragged(v, block, kind, route, parts[0].plan, per_frame);
        std::vector<RFrame> emb(v), map(v);
        for (size_t i = 0; i < v.size(); ++i) {
            emb[i].out2 = nullptr;
            map[i].in1 = nullptr;
            map[i].out = v[i].out2;
            map[i].out2 = nullptr;
        }
        plan_ragged(emb, block, RKind::Embed, route, parts[0].plan, per_frame);  // (the map takes no alpha)
        plan_ragged(map, block, RKind::Map, TMFWM_ROUTE_HYBRID, parts[1].plan);
    };
    int64_t total_n = 0, total_list = 0;
    if (mem_kind == TMFWM_MEM_DEVICE) {
        if (int rc = check_ragged_device(fr, block, kind)) return rc;
        plan_parts(fr);
        for (Part &p : parts) {
            t_list_pass = 0;
            if (int rc = run_ragged(block, alpha, st, device_report(n_lapack ? &p.n : nullptr), p.plan, px)) return rc;
            total_n += p.n;
            total_list += t_list_pass;
        }
        if (n_lapack) {
            *n_lapack = total_n;
            t_list_pass = total_list;
        }
        return 0;
    }
    // host memory: every buffer of the call in one device allocation (16-byte aligned pieces),
    // results copied back, one synchronisation
    std::vector<RFrame> dv(fr);
    size_t total = 0;
    std::vector<size_t> off(fr.size() * 3), off2(fr.size());
    for (size_t i = 0; i < fr.size(); ++i) {
        const size_t sz[3] = {(size_t)fr[i].pixel_bytes(), (size_t)fr[i].in1_bytes(kind, block), (size_t)fr[i].out_bytes(kind, block)};
        for (int k = 0; k < 3; ++k) {
            off[3 * i + k] = total;
            total += round16(sz[k]);
        }
        off2[i] = total;
        total += round16((size_t)fr[i].out2_bytes(kind, block));
    }
    DevBuf stage;
    if (int rc = stage.alloc(total, st, "ragged frames")) return rc;
    uint8_t *base = static_cast<uint8_t *>(stage.p);
    for (size_t i = 0; i < fr.size(); ++i) {
        const size_t ib = (size_t)fr[i].in1_bytes(kind, block);
        if (!fr[i].has_work(kind, block)) continue;
        dv[i].in0 = base + off[3 * i];
        dv[i].in1 = ib ? base + off[3 * i + 1] : nullptr;
        dv[i].out = base + off[3 * i + 2];
        dv[i].out2 = fr[i].out2_bytes(kind, block) ? base + off2[i] : nullptr;
        TMF_HIP(hipMemcpyAsync(base + off[3 * i], fr[i].in0, (size_t)fr[i].pixel_bytes(), hipMemcpyHostToDevice, st));
        if (ib) TMF_HIP(hipMemcpyAsync(base + off[3 * i + 1], fr[i].in1, ib, hipMemcpyHostToDevice, st));
    }
    plan_parts(dv);
    std::vector<std::unique_ptr<HostCall>> hc;
    for (Part &p : parts) {
        hc.emplace_back(new HostCall((int64_t)p.plan.chunks.size(), st, &p.n));
        t_list_pass = 0;
        if (int rc = run_ragged(block, alpha, st, hc.back()->report(), p.plan, px)) return rc;
        if (!hc.back()->sink.p) total_list += t_list_pass;  // read back by the passes themselves
    }
    for (size_t i = 0; i < fr.size(); ++i) {
        if (!fr[i].has_work(kind, block)) continue;
        TMF_HIP(hipMemcpyAsync(fr[i].out, dv[i].out, (size_t)fr[i].out_bytes(kind, block), hipMemcpyDeviceToHost, st));
        if (const size_t kb = (size_t)fr[i].out2_bytes(kind, block))
            TMF_HIP(hipMemcpyAsync(fr[i].out2, dv[i].out2, kb, hipMemcpyDeviceToHost, st));
    }
    for (size_t k = 0; k < parts.size(); ++k) {
        if (int rc = hc[k]->finish()) return rc;
        if (hc[k]->sink.p && hc[k]->nchunks) total_list += t_list_pass;
        total_n += parts[k].n;
    }
    if (n_lapack) *n_lapack = total_n;
    t_list_pass = total_list;
    return 0;
}

// ---- ragged tile preparation (tmfwm_tile_plan.h)

// TMFWM_DEBUG_TILE_SCRATCH (bytes) lowers the bound of a group's scratch so that the tests can
// run several groups at small sizes
int64_t tile_scratch_cap()
{
    const char *e = std::getenv("TMFWM_DEBUG_TILE_SCRATCH");
    if (!e || !*e) return tmf::kTileScratchCap;
    const long long v = std::atoll(e);
    return v > 0 && v < tmf::kTileScratchCap ? (int64_t)v : tmf::kTileScratchCap;
}

// The plan's job table and packed tables built in one pinned buffer, uploaded in one copy, then
// two launches per group (one where no job of the group needs the horizontal pass).  Nothing here
// waits for the stream.
int run_tiles_ragged(const tmf::TilePlan &plan, hipStream_t st)
{
    const size_t jbytes = plan.jobs.size() * sizeof(tmf::TileJob), tbytes = plan.tables.size() * sizeof(int);
    TableSlot slot;
    if (int rc = take_table(jbytes + tbytes, stream_device(st), slot)) return rc;
    std::copy(plan.jobs.begin(), plan.jobs.end(), static_cast<tmf::TileJob *>(slot.p));
    std::copy(plan.tables.begin(), plan.tables.end(), reinterpret_cast<int *>(static_cast<uint8_t *>(slot.p) + jbytes));
    DevBuf dtab, dtmp;
    int rc = dtab.alloc(jbytes + tbytes, st, "tile jobs and resample tables");
    if (rc == 0 && hipMemcpyAsync(dtab.p, slot.p, jbytes + tbytes, hipMemcpyHostToDevice, st) != hipSuccess)
        rc = fail(TMFWM_ERR_HIP, "copying the tile jobs and resample tables failed: %s", hipGetErrorString(hipGetLastError()));
    give_table(slot, st);
    if (rc) return rc;
    if (int rc2 = dtmp.alloc((size_t)plan.scratch, st, "resample scratch")) return rc2;
    const tmf::TileJob *djobs = static_cast<const tmf::TileJob *>(dtab.p);
    const int *dtables = reinterpret_cast<const int *>(static_cast<const uint8_t *>(dtab.p) + jbytes);
    for (const tmf::TileGroup &g : plan.groups)  // in stream order: the groups share the scratch
        TMF_HIP(tmf::launch_tiles_ragged(djobs + g.first, g.n, dtables, static_cast<uint8_t *>(dtmp.p), g.h_items, g.v_items, st));
    return 0;
}

int tiles_ragged_call(std::vector<tmf::TileJobIn> &jobs, bool preserve_ratio, int32_t mem_kind, void *hip_stream)
{
    // sizes, the resized size and the pointers of every job, before the device is touched
    for (size_t i = 0; i < jobs.size(); ++i) {
        const tmf::TileJobIn &j = jobs[i];
        tmf::TileGeom geo;
        if (j.wh <= 0 || j.ww <= 0 || j.th <= 0 || j.tw <= 0)
            return fail(TMFWM_ERR_INVALID, "job %zu: height and width must be > 0 (watermark %dx%d, tile %dx%d)", i, j.ww, j.wh, j.tw,
                        j.th);
        if (!tmf::tile_geom(j.wh, j.ww, j.th, j.tw, preserve_ratio, geo))
            return fail(TMFWM_ERR_INVALID, "job %zu: height and width must be > 0 (resized %dx%d)", i, geo.rw, geo.rh);
        if (!j.wm || !j.tile) return fail(TMFWM_ERR_INVALID, "job %zu: NULL pointer in the descriptor", i);
    }
    if (int rc = need_device()) return rc;
    if (jobs.empty()) return 0;
    hipStream_t st = pick_stream(hip_stream);
    DevBuf stage;
    std::vector<uint8_t *> host_tile;
    if (mem_kind == TMFWM_MEM_DEVICE) {
        std::vector<Span> spans;
        spans.reserve(jobs.size() * 2);
        for (size_t i = 0; i < jobs.size(); ++i) {
            const tmf::TileJobIn &j = jobs[i];
            if (int rc = check_device_ptr(j.wm, "wm")) return fail(rc, "job %zu: %s", i, t_err.c_str());
            if (int rc = check_device_ptr(j.tile, "tile")) return fail(rc, "job %zu: %s", i, t_err.c_str());
            const uintptr_t w = reinterpret_cast<uintptr_t>(j.wm), t = reinterpret_cast<uintptr_t>(j.tile);
            spans.push_back({w, w + (uintptr_t)j.wh * (uintptr_t)j.ww, false, (int64_t)i});
            spans.push_back({t, t + (uintptr_t)j.th * (uintptr_t)j.tw, true, (int64_t)i});
        }
        if (int rc = check_ragged_overlap(spans, "job")) return rc;
    } else {  // host memory: every watermark and tile staged compactly in one device allocation (16-byte aligned pieces)
        size_t total = 0;
        std::vector<size_t> off(jobs.size() * 2);
        for (size_t i = 0; i < jobs.size(); ++i) {
            off[2 * i] = total;
            total += round16((size_t)jobs[i].wh * (size_t)jobs[i].ww);
            off[2 * i + 1] = total;
            total += round16((size_t)jobs[i].th * (size_t)jobs[i].tw);
        }
        if (int rc = stage.alloc(total, st, "watermarks and tiles")) return rc;
        uint8_t *base = static_cast<uint8_t *>(stage.p);
        host_tile.resize(jobs.size());
        for (size_t i = 0; i < jobs.size(); ++i) {
            TMF_HIP(hipMemcpyAsync(base + off[2 * i], jobs[i].wm, (size_t)jobs[i].wh * (size_t)jobs[i].ww, hipMemcpyHostToDevice, st));
            host_tile[i] = jobs[i].tile;
            jobs[i].wm = base + off[2 * i];
            jobs[i].tile = base + off[2 * i + 1];
        }
    }
    tmf::TilePlan plan;
    const char *why = "";
    int64_t bad = -1;
    try {
        bad = plan.build(jobs.data(), (int64_t)jobs.size(), preserve_ratio, tile_scratch_cap(), &why);
    } catch (const std::bad_alloc &) {
        return fail(TMFWM_ERR_NOMEM, "host allocation for the resample tables failed");
    }
    if (bad >= 0) return fail(TMFWM_ERR_INVALID, "job %lld: %s", (long long)bad, why);
    if (int rc = run_tiles_ragged(plan, st)) return rc;
    if (mem_kind == TMFWM_MEM_HOST) {
        for (size_t i = 0; i < jobs.size(); ++i)
            TMF_HIP(hipMemcpyAsync(host_tile[i], jobs[i].tile, (size_t)jobs[i].th * (size_t)jobs[i].tw, hipMemcpyDeviceToHost, st));
        TMF_HIP(hipStreamSynchronize(st));  // the tiles have landed
    }
    return 0;
}

}  // namespace
}  // extern "C++"

int tmfwm_embed_ragged(const tmfwm_embed_frame *frames, int64_t n_frames, int32_t block, double alpha, int32_t mem_kind,
                       void *hip_stream, int32_t route, int64_t *n_lapack_blocks)
{
    if (int rc = check_ragged_call(frames, n_frames, block, alpha, RKind::Embed, mem_kind, route, n_lapack_blocks)) return rc;
    std::vector<RFrame> fr((size_t)n_frames);  // the library's copy: the caller's array is not read again
    for (int64_t i = 0; i < n_frames; ++i) fr[(size_t)i] = {frames[i].rgb, frames[i].wm_tile, frames[i].out, frames[i].height, frames[i].width};
    return ragged_call(fr, block, alpha, RKind::Embed, mem_kind, hip_stream, route, n_lapack_blocks);
}

int tmfwm_embed_key_ragged(const tmfwm_embed_key_frame *frames, int64_t n_frames, int32_t block, double alpha, int32_t mem_kind,
                           void *hip_stream, int32_t route, int64_t *n_lapack_blocks)
{
    if (int rc = check_ragged_call(frames, n_frames, block, alpha, RKind::EmbedKey, mem_kind, route, n_lapack_blocks)) return rc;
    std::vector<RFrame> fr((size_t)n_frames);
    for (int64_t i = 0; i < n_frames; ++i)
        fr[(size_t)i] = {frames[i].rgb, frames[i].wm_tile, frames[i].out, frames[i].height, frames[i].width,
                         reinterpret_cast<uint8_t *>(frames[i].out_key)};
    return ragged_call(fr, block, alpha, RKind::EmbedKey, mem_kind, hip_stream, route, n_lapack_blocks);
}

int tmfwm_embed_ragged_rank1(const tmfwm_embed_frame *frames, int64_t n_frames, int32_t block, double alpha, int32_t mem_kind,
                             void *hip_stream, int32_t route, int64_t *n_lapack_blocks)
{
    if (int rc = check_ragged_call(frames, n_frames, block, alpha, RKind::Embed, mem_kind, route, n_lapack_blocks, true)) return rc;
    std::vector<RFrame> fr((size_t)n_frames);
    for (int64_t i = 0; i < n_frames; ++i) fr[(size_t)i] = {frames[i].rgb, frames[i].wm_tile, frames[i].out, frames[i].height, frames[i].width};
    return ragged_call(fr, block, alpha, RKind::Embed, mem_kind, hip_stream, route, n_lapack_blocks);
}

int tmfwm_embed_key_ragged_rank1(const tmfwm_embed_key_frame *frames, int64_t n_frames, int32_t block, double alpha, int32_t mem_kind,
                                 void *hip_stream, int32_t route, int64_t *n_lapack_blocks)
{
    if (int rc = check_ragged_call(frames, n_frames, block, alpha, RKind::EmbedKey, mem_kind, route, n_lapack_blocks, true)) return rc;
    std::vector<RFrame> fr((size_t)n_frames);
    for (int64_t i = 0; i < n_frames; ++i)
        fr[(size_t)i] = {frames[i].rgb, frames[i].wm_tile, frames[i].out, frames[i].height, frames[i].width,
                         reinterpret_cast<uint8_t *>(frames[i].out_key)};
    return ragged_call(fr, block, alpha, RKind::EmbedKey, mem_kind, hip_stream, route, n_lapack_blocks);
}

int tmfwm_extract_ragged(const tmfwm_extract_frame *frames, int64_t n_frames, int32_t block, double alpha, int32_t mem_kind,
                         void *hip_stream, int32_t route, int64_t *n_lapack_blocks)
{
    if (int rc = check_ragged_call(frames, n_frames, block, alpha, RKind::Extract, mem_kind, route, n_lapack_blocks)) return rc;
    std::vector<RFrame> fr((size_t)n_frames);
    for (int64_t i = 0; i < n_frames; ++i)
        fr[(size_t)i] = {frames[i].wm_rgb, frames[i].orig_rgb, frames[i].out_tile, frames[i].height, frames[i].width};
    return ragged_call(fr, block, alpha, RKind::Extract, mem_kind, hip_stream, route, n_lapack_blocks);
}

// keyed extraction over ragged batches: the key rides in the frame's in1 / out slot as bytes; every
// frame of the call holds pixel_bytes bytes per pixel
int tmfwm_sigma1_map_ragged_px(const tmfwm_key_frame *frames, int64_t n_frames, int32_t block, int32_t pixel_bytes, int32_t mem_kind,
                               void *hip_stream, int32_t route, int64_t *n_lapack_blocks)
{
    if (int rc = check_ragged_call(frames, n_frames, block, 1.0, RKind::Map, mem_kind, route, n_lapack_blocks)) return rc;
    if (pixel_bytes != TMFWM_PIX_RGB && pixel_bytes != TMFWM_PIX_RGBX) return fail(TMFWM_ERR_INVALID, "pixel bytes %d (3 or 4)", pixel_bytes);
    std::vector<RFrame> fr((size_t)n_frames);
    for (int64_t i = 0; i < n_frames; ++i)
        fr[(size_t)i] = {frames[i].rgb, nullptr,    reinterpret_cast<uint8_t *>(frames[i].out_key), frames[i].height, frames[i].width,
                         nullptr,       pixel_bytes};
    return ragged_call(fr, block, 1.0, RKind::Map, mem_kind, hip_stream, route, n_lapack_blocks);
}

int tmfwm_sigma1_map_ragged(const tmfwm_key_frame *frames, int64_t n_frames, int32_t block, int32_t mem_kind, void *hip_stream,
                            int32_t route, int64_t *n_lapack_blocks)
{
    return tmfwm_sigma1_map_ragged_px(frames, n_frames, block, TMFWM_PIX_RGB, mem_kind, hip_stream, route, n_lapack_blocks);
}

int tmfwm_extract_keyed_ragged_px(const tmfwm_keyed_frame *frames, int64_t n_frames, int32_t block, double alpha, int32_t pixel_bytes,
                                  int32_t mem_kind, void *hip_stream, int32_t route, int64_t *n_lapack_blocks)
{
    if (int rc = check_ragged_call(frames, n_frames, block, alpha, RKind::Keyed, mem_kind, route, n_lapack_blocks)) return rc;
    if (pixel_bytes != TMFWM_PIX_RGB && pixel_bytes != TMFWM_PIX_RGBX) return fail(TMFWM_ERR_INVALID, "pixel bytes %d (3 or 4)", pixel_bytes);
    std::vector<RFrame> fr((size_t)n_frames);
    for (int64_t i = 0; i < n_frames; ++i)
        fr[(size_t)i] = {frames[i].wm_rgb, reinterpret_cast<const uint8_t *>(frames[i].key), frames[i].out_tile, frames[i].height,
                         frames[i].width,  nullptr, pixel_bytes};
    return ragged_call(fr, block, alpha, RKind::Keyed, mem_kind, hip_stream, route, n_lapack_blocks);
}

int tmfwm_extract_keyed_ragged(const tmfwm_keyed_frame *frames, int64_t n_frames, int32_t block, double alpha, int32_t mem_kind,
                               void *hip_stream, int32_t route, int64_t *n_lapack_blocks)
{
    return tmfwm_extract_keyed_ragged_px(frames, n_frames, block, alpha, TMFWM_PIX_RGB, mem_kind, hip_stream, route, n_lapack_blocks);
}

// one alpha per frame: the uniform calls' checks, then every alpha, then the same ragged_call with
// each frame's alpha in its RFrame (copied, as the descriptors are, before the call returns); a
// call without a frame is done once its arguments are checked
int tmfwm_embed_ragged_alphas(const tmfwm_embed_frame *frames, const double *alphas, int64_t n_frames, int32_t block, int32_t mem_kind,
                              void *hip_stream, int32_t route, int64_t *n_lapack_blocks)
{
    if (int rc = check_ragged_call(frames, n_frames, block, 1.0, RKind::Embed, mem_kind, route, n_lapack_blocks, true)) return rc;
    if (int rc = check_ragged_alphas(alphas, n_frames, RKind::Embed)) return rc;
    if (n_frames == 0) return 0;
    std::vector<RFrame> fr((size_t)n_frames);
    for (int64_t i = 0; i < n_frames; ++i) {
        fr[(size_t)i] = RFrame{frames[i].rgb, frames[i].wm_tile, frames[i].out, frames[i].height, frames[i].width};
        fr[(size_t)i].alpha = alphas[i];
    }
    return ragged_call(fr, block, 0.0, RKind::Embed, mem_kind, hip_stream, route, n_lapack_blocks, true);
}

int tmfwm_embed_key_ragged_alphas(const tmfwm_embed_key_frame *frames, const double *alphas, int64_t n_frames, int32_t block,
                                  int32_t mem_kind, void *hip_stream, int32_t route, int64_t *n_lapack_blocks)
{
    if (int rc = check_ragged_call(frames, n_frames, block, 1.0, RKind::EmbedKey, mem_kind, route, n_lapack_blocks, true)) return rc;
    if (int rc = check_ragged_alphas(alphas, n_frames, RKind::EmbedKey)) return rc;
    if (n_frames == 0) return 0;
    std::vector<RFrame> fr((size_t)n_frames);
    for (int64_t i = 0; i < n_frames; ++i) {
        fr[(size_t)i] = RFrame{frames[i].rgb, frames[i].wm_tile, frames[i].out, frames[i].height, frames[i].width,
                               reinterpret_cast<uint8_t *>(frames[i].out_key)};
        fr[(size_t)i].alpha = alphas[i];
    }
    return ragged_call(fr, block, 0.0, RKind::EmbedKey, mem_kind, hip_stream, route, n_lapack_blocks, true);
}

int tmfwm_extract_ragged_alphas(const tmfwm_extract_frame *frames, const double *alphas, int64_t n_frames, int32_t block,
                                int32_t mem_kind, void *hip_stream, int32_t route, int64_t *n_lapack_blocks)
{
    if (int rc = check_ragged_call(frames, n_frames, block, 1.0, RKind::Extract, mem_kind, route, n_lapack_blocks)) return rc;
    if (int rc = check_ragged_alphas(alphas, n_frames, RKind::Extract)) return rc;
    if (n_frames == 0) return 0;
    std::vector<RFrame> fr((size_t)n_frames);
    for (int64_t i = 0; i < n_frames; ++i) {
        fr[(size_t)i] = RFrame{frames[i].wm_rgb, frames[i].orig_rgb, frames[i].out_tile, frames[i].height, frames[i].width};
        fr[(size_t)i].alpha = alphas[i];
    }
    return ragged_call(fr, block, 1.0, RKind::Extract, mem_kind, hip_stream, route, n_lapack_blocks, true);
}

int tmfwm_extract_keyed_ragged_alphas(const tmfwm_keyed_frame *frames, const double *alphas, int64_t n_frames, int32_t block,
                                      int32_t pixel_bytes, int32_t mem_kind, void *hip_stream, int32_t route, int64_t *n_lapack_blocks)
{
    if (int rc = check_ragged_call(frames, n_frames, block, 1.0, RKind::Keyed, mem_kind, route, n_lapack_blocks)) return rc;
    if (int rc = check_ragged_alphas(alphas, n_frames, RKind::Keyed)) return rc;
    if (pixel_bytes != TMFWM_PIX_RGB && pixel_bytes != TMFWM_PIX_RGBX) return fail(TMFWM_ERR_INVALID, "pixel bytes %d (3 or 4)", pixel_bytes);
    if (n_frames == 0) return 0;
    std::vector<RFrame> fr((size_t)n_frames);
    for (int64_t i = 0; i < n_frames; ++i)
        fr[(size_t)i] = {frames[i].wm_rgb, reinterpret_cast<const uint8_t *>(frames[i].key), frames[i].out_tile, frames[i].height,
                         frames[i].width,  nullptr, pixel_bytes, alphas[i]};
    return ragged_call(fr, block, 1.0, RKind::Keyed, mem_kind, hip_stream, route, n_lapack_blocks, true);
}

int tmfwm_prepare_tiles_ragged(const tmfwm_tile_job *jobs, int64_t n_jobs, int32_t preserve_ratio, int32_t mem_kind,
                               void *hip_stream)
{
    t_err.clear();
    if (n_jobs < 0) return fail(TMFWM_ERR_INVALID, "negative size (n_jobs=%lld)", (long long)n_jobs);
    if (n_jobs > 0 && !jobs) return fail(TMFWM_ERR_INVALID, "jobs is NULL");
    if (mem_kind != TMFWM_MEM_HOST && mem_kind != TMFWM_MEM_DEVICE) return fail(TMFWM_ERR_INVALID, "mem_kind %d", mem_kind);
    std::vector<tmf::TileJobIn> in((size_t)n_jobs);  // the library's copy: the caller's array is not read again
    for (int64_t i = 0; i < n_jobs; ++i)
        in[(size_t)i] = {jobs[i].wm, jobs[i].tile, jobs[i].wm_height, jobs[i].wm_width, jobs[i].tile_height, jobs[i].tile_width};
    return tiles_ragged_call(in, preserve_ratio != 0, mem_kind, hip_stream);
}

}  // extern "C"
