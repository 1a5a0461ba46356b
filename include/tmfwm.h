/*
 * tmfwm.h -- C ABI of libtmfwm.so, the MI355X (gfx950) implementation of the
 * block-wise DCT+SVD watermark path of ThatsMyFace (modules/watermarking.py).
 *
 * Drop-in boundary: the reference's Python functions keep their signatures
 * (thatsmyface_amd/watermarking.py mirrors them); underneath, each per-pixel /
 * per-block loop of the reference becomes one call below.  Plain pointers and
 * sizes only.  The caller owns every buffer.  No exceptions cross the ABI.
 *
 * Status codes: 0 ok, negative errno-style values on error; the thread-local
 * message is available from tmfwm_last_error().  All entry points are
 * re-entrant (Streamlit runs sessions on threads): no mutable global state,
 * per-call or per-thread HIP streams.
 *
 * Memory: mem_kind = TMFWM_MEM_DEVICE -> every pointer is device memory of the
 * current HIP device (e.g. a torch tensor's data_ptr()); work is enqueued on
 * `hip_stream` (NULL = the per-thread default stream) and the call returns
 * without synchronising.  mem_kind = TMFWM_MEM_HOST -> pointers are host
 * memory; the library stages through device memory and returns after the
 * results are back in host memory.
 *
 * Image layout: n_frames frames of height x width x 3 uint8, HWC interleaved
 * (numpy / PIL "RGB" order), frame i at base + i * frame_stride bytes
 * (frame_stride >= height*width*3).  Block grid: nbh = height / block,
 * nbw = width / block.  Supported block sizes: 4, 6, 8, 10, 12, 14, 16 -- the app's
 * slider values (others return TMFWM_ERR_UNSUPPORTED).
 *
 * SVD routes: every block goes through a fused Jacobi SVD; the
 * blocks whose factors could round differently from LAPACK's (conditioning test) and,
 * since ABI 9, every block whose output bytes the byte certificate cannot prove equal to
 * LAPACK's (interval arithmetic through the reconstruct, IDCT and inverse colour) are
 * redone by a second pass on the dgesdd route -- numpy's np.linalg.svd restated
 * operation by operation (LAPACK 3.12 + OpenBLAS 0.3.29 SkylakeX kernels) -- so the
 * bytes are the reference's.  The _ex entry points report how many blocks took it.
 */
#ifndef TMFWM_H
#define TMFWM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TMFWM_ABI_VERSION 10

#define TMFWM_MEM_HOST 0
#define TMFWM_MEM_DEVICE 1

/* SVD routes of embed / extract (tmfwm_embed_route, tmfwm_extract_route) */
#define TMFWM_ROUTE_HYBRID 0    /* Jacobi on every block, the dgesdd route for the blocks the
                                   conditioning test flags or whose bytes the certificate cannot
                                   prove (the throughput route: tmfwm_embed) */
#define TMFWM_ROUTE_REFERENCE 1 /* the dgesdd route -- np.linalg.svd's own arithmetic -- for every
                                   block: the reference's bytes by construction */
#define TMFWM_ROUTE_RANK1 2     /* (ABI 10) embed: a rank-1 pre-pass keeps the bytes of every
                                   block whose f32(D + c u1 v1^T) it proves equal to the reference's
                                   (photo mode) and sends the rest through the hybrid
                                   route (every slider size, b = 4..16 even); extract:
                                   TMFWM_ROUTE_HYBRID */
#define TMFWM_ROUTE_RANK1_REFERENCE 3 /* (ABI 10) the same pre-pass in front of the dgesdd route: no
                                   Jacobi SVD and so no K -- embed rests on the pre-pass's rank-one
                                   bound (its constants on LAPACK's residual and top pair enter
                                   scaled by ~2^-24), extract on the certified sigma_1 enclosure
                                   (TMFWM_ROUTE_HYBRID's extract); every slider size */

#define TMFWM_OK 0
#define TMFWM_ERR_INVALID (-22)     /* bad argument (EINVAL) */
#define TMFWM_ERR_NOMEM (-12)       /* device allocation failed (ENOMEM) */
#define TMFWM_ERR_HIP (-5)          /* HIP runtime / launch error (EIO) */
#define TMFWM_ERR_UNSUPPORTED (-95) /* block size not an even 4..16 (EOPNOTSUPP) */
#define TMFWM_ERR_NODEVICE (-19)    /* no usable gfx950 device (ENODEV) */
#define TMFWM_ERR_NODATA (-61)      /* no decodable QR code in the image (ENODATA) */

/* ABI version (TMFWM_ABI_VERSION) compiled into the library. */
int tmfwm_abi_version(void);

/* Message of the last failed call on this thread ("" if none). */
const char *tmfwm_last_error(void);

/* Work report of the last tmfwm_embed_ex / tmfwm_extract_ex call on this thread that asked
 * for one (non-NULL n_lapack_blocks): the number of blocks the strip pass left to the list
 * pass -- embed: blocks needing more f64 Jacobi sweeps than the rest of their wave (DESIGN.md
 * 4); extract: blocks whose sigma_1 the strip pass's power iterations did not decide (DESIGN.md
 * 5); -1 before any such call.  Diagnostics only: the output does not depend on it. */
int64_t tmfwm_last_list_pass_blocks(void);

/* 1 when tmfwm_embed at this block size runs a list pass after its strip pass (the strip pass
 * may leave blocks that need more f64 Jacobi sweeps than the rest of their wave to it,
 * DESIGN.md 4), else 0 (also for unsupported sizes).  Describes the launches of a call; the
 * output does not depend on it.  (ABI 7) */
int tmfwm_embed_list_pass(int32_t block);

/* Number of visible HIP devices (0 when none); never fails. */
int tmfwm_device_count(void);

/*
 * Embed: replaces the body of embed_watermark() (watermarking.py:163-219):
 * RGB->YCbCr (:166), per-block 2-D DCT (:192), SVD (:195), S[0] += alpha*w/255
 * (:198), U diag(S) Vt (:201), IDCT (:204), write-back (:207-213), YCbCr->RGB
 * (:216).  wm_tile is the already-resized watermark (resize_watermark :86,
 * host side), nbh x nbw uint8, shared by all frames.  out may not alias rgb.
 */
int tmfwm_embed(const uint8_t *rgb, int64_t n_frames, int32_t height, int32_t width, int64_t frame_stride,
                const uint8_t *wm_tile, int32_t block, double alpha, uint8_t *out, int32_t mem_kind, void *hip_stream);

/*
 * tmfwm_embed with a report: *n_lapack_blocks (optional, host pointer) receives the
 * number of blocks that took the dgesdd route.  Passing it makes the call wait for
 * `hip_stream` (the count lives on the device); NULL keeps TMFWM_MEM_DEVICE calls
 * asynchronous.
 *
 * A dgesdd-route block on which dbdsqr does not converge (np.linalg.svd raises LinAlgError
 * there) fails the call with TMFWM_ERR_HIP whenever the call synchronises: every
 * TMFWM_MEM_HOST call, and every call with a non-NULL n_lapack_blocks.  An asynchronous
 * TMFWM_MEM_DEVICE call without a count pointer cannot report it (the same holds for extract).
 */
int tmfwm_embed_ex(const uint8_t *rgb, int64_t n_frames, int32_t height, int32_t width, int64_t frame_stride,
                   const uint8_t *wm_tile, int32_t block, double alpha, uint8_t *out, int32_t mem_kind, void *hip_stream,
                   int64_t *n_lapack_blocks);

/*
 * tmfwm_embed_ex with an explicit SVD route (ABI 7): TMFWM_ROUTE_HYBRID is tmfwm_embed_ex;
 * TMFWM_ROUTE_REFERENCE sends every block through the dgesdd route (LAPACK dgesdd + the
 * OpenBLAS kernels numpy calls, restated operation by operation), so each output byte is
 * computed by the reference's own arithmetic, with no certificate and no error bound to rely
 * on (the hybrid route's bytes equal it through its byte certificate, which rests on one
 * measured bound).  About two orders of magnitude less
 * throughput than the hybrid route; *n_lapack_blocks then counts every block.
 * TMFWM_ROUTE_RANK1 (ABI 10): the hybrid route behind a rank-1 pre-pass (b = 4..16; photographs,
 * whose blocks it mostly decides alone); tmfwm_last_list_pass_blocks() then counts the blocks
 * it left to the hybrid route.
 */
int tmfwm_embed_route(const uint8_t *rgb, int64_t n_frames, int32_t height, int32_t width, int64_t frame_stride,
                      const uint8_t *wm_tile, int32_t block, double alpha, uint8_t *out, int32_t mem_kind, void *hip_stream,
                      int32_t route, int64_t *n_lapack_blocks);

/*
 * Extract: replaces the body of extract_watermark() (watermarking.py:246-292):
 * luma of both images, per-block sigma_1 of the DCT of each, (s_w - s_o)/alpha
 * in float32, clip to [0,1], *255, truncation.  Both images have the same
 * height x width (the caller crops a larger original, as the reference's
 * slicing does).  out_tiles: n_frames tiles of nbh x nbw uint8, back to back.
 */
int tmfwm_extract(const uint8_t *wm_rgb, const uint8_t *orig_rgb, int64_t n_frames, int32_t height, int32_t width,
                  int64_t frame_stride, int32_t block, double alpha, uint8_t *out_tiles, int32_t mem_kind,
                  void *hip_stream);

/* tmfwm_extract with a report: *n_lapack_blocks (optional) receives the number of
 * blocks whose sigma_1 pair was computed on the dgesdd route (the rest are certified). */
int tmfwm_extract_ex(const uint8_t *wm_rgb, const uint8_t *orig_rgb, int64_t n_frames, int32_t height, int32_t width,
                     int64_t frame_stride, int32_t block, double alpha, uint8_t *out_tiles, int32_t mem_kind,
                     void *hip_stream, int64_t *n_lapack_blocks);

/* tmfwm_extract_ex with an explicit SVD route (ABI 7): TMFWM_ROUTE_REFERENCE computes both
 * sigma_1 of every block on the dgesdd route instead of certifying the Jacobi enclosure. */
int tmfwm_extract_route(const uint8_t *wm_rgb, const uint8_t *orig_rgb, int64_t n_frames, int32_t height, int32_t width,
                        int64_t frame_stride, int32_t block, double alpha, uint8_t *out_tiles, int32_t mem_kind,
                        void *hip_stream, int32_t route, int64_t *n_lapack_blocks);

/*
 * Keyed extraction (added within ABI 10; the version number is unchanged and existing entry
 * points keep their behaviour).  Extract uses the original image for one number per block only:
 * f32(sigma_1) of the block's DCT.  tmfwm_sigma1_map computes that number for every block of
 * every frame -- the key: (height/block) x (width/block) float32 per frame, n_frames maps back to
 * back in out_key -- and tmfwm_extract_keyed extracts from the watermarked frames and a key
 * instead of the original's pixels.  Its bytes are exactly tmfwm_extract_route's for the original
 * the key was made from.  A key belongs to one block size and one image size.
 *
 * key_stride: bytes between consecutive frames' keys; 0 is one key shared by every frame (one
 * original, many watermarked copies), any other value must be a multiple of 4 and
 * >= (height/block)*(width/block)*4 (TMFWM_ERR_INVALID otherwise).  A key entry that is not
 * finite gives byte 0.
 *
 * Routes as tmfwm_extract_route: TMFWM_ROUTE_REFERENCE computes every sigma_1 on the dgesdd
 * route, the others certify the enclosure and send the undecided blocks there; a key entry is
 * np.linalg.svd's float32 S[0] on every route, so keys do not depend on the route.
 * *n_lapack_blocks, tmfwm_last_list_pass_blocks(), the non-convergence report, TMFWM_MEM_HOST
 * staging and TMFWM_MEM_DEVICE asynchrony as tmfwm_extract_route; with TMFWM_MEM_DEVICE the
 * output must not overlap an input.  Pixels are 3 bytes (TMFWM_PIX_RGB); tmfwm_sigma1_map_px and
 * tmfwm_extract_keyed_px below take 4-byte pixels as well.
 */
int tmfwm_sigma1_map(const uint8_t *rgb, int64_t n_frames, int32_t height, int32_t width, int64_t frame_stride,
                     int32_t block, float *out_key, int32_t mem_kind, void *hip_stream, int32_t route,
                     int64_t *n_lapack_blocks);
int tmfwm_extract_keyed(const uint8_t *wm_rgb, int64_t n_frames, int32_t height, int32_t width, int64_t frame_stride,
                        const float *key, int64_t key_stride, int32_t block, double alpha, uint8_t *out_tiles,
                        int32_t mem_kind, void *hip_stream, int32_t route, int64_t *n_lapack_blocks);

/* Pixel layouts of tmfwm_embed_px / tmfwm_extract_px (ABI 8) */
#define TMFWM_PIX_RGB 3  /* 3 bytes per pixel, R G B (numpy / Image.tobytes order) */
#define TMFWM_PIX_RGBX 4 /* 4 bytes per pixel, R G B pad: how PIL holds a mode-"RGB" image in memory
                            (Image.__arrow_c_array__ / Image.fromarrow share it without a copy);
                            the pad byte is ignored on input and written as 255 */

/*
 * tmfwm_sigma1_map and tmfwm_extract_keyed with a pixel layout (added within ABI 10; the version
 * number is unchanged and existing entry points keep their behaviour): the frames hold
 * pixel_bytes per pixel (TMFWM_PIX_RGB or TMFWM_PIX_RGBX; anything else is TMFWM_ERR_INVALID)
 * and lie frame_stride bytes apart, frame_stride >= height*width*pixel_bytes.  Key bits and tile
 * bytes are exactly those of the 3-byte call on the same R, G, B values; the pad byte is ignored.
 * The keyed calls only read pixels, so 4-byte frames are read where they lie: kernels of their own
 * take the R G B pad rows (whole dwords at every block size once the frames' base and
 * frame_stride are multiples of 4, bytes otherwise), and with TMFWM_MEM_HOST the frames are
 * staged as they are -- no pack launch and no 3-byte staging buffer.  With pixel_bytes == 3 each
 * call is its sibling above.  Routes, *n_lapack_blocks, tmfwm_last_list_pass_blocks(), the
 * non-convergence report, chunking, key_stride, the overlap rule and the alignment of out_key /
 * key (4 bytes) as there; all arguments are checked before the device is touched.
 */
int tmfwm_sigma1_map_px(const uint8_t *rgb, int32_t pixel_bytes, int64_t frame_stride, int64_t n_frames, int32_t height,
                        int32_t width, int32_t block, float *out_key, int32_t mem_kind, void *hip_stream, int32_t route,
                        int64_t *n_lapack_blocks);
int tmfwm_extract_keyed_px(const uint8_t *wm_rgb, int32_t pixel_bytes, int64_t frame_stride, int64_t n_frames, int32_t height,
                           int32_t width, const float *key, int64_t key_stride, int32_t block, double alpha,
                           uint8_t *out_tiles, int32_t mem_kind, void *hip_stream, int32_t route, int64_t *n_lapack_blocks);

/*
 * tmfwm_embed_route with a pixel layout per side (ABI 8): the input frames have
 * in_pixel_bytes per pixel (TMFWM_PIX_*) and in_frame_stride bytes between frames, the
 * output out_pixel_bytes and out_frame_stride.  The bytes of every pixel's R, G, B are
 * tmfwm_embed's.  4-byte frames are converted on the device, so the drop-in hands PIL's
 * own image memory to the library and wraps the output as an image without a host-side
 * pack or unpack.  3 -> 3 is tmfwm_embed_route (one frame stride for both).
 */
int tmfwm_embed_px(const uint8_t *rgb, int32_t in_pixel_bytes, int64_t in_frame_stride, int64_t n_frames, int32_t height,
                   int32_t width, const uint8_t *wm_tile, int32_t block, double alpha, uint8_t *out, int32_t out_pixel_bytes,
                   int64_t out_frame_stride, int32_t mem_kind, void *hip_stream, int32_t route, int64_t *n_lapack_blocks);

/*
 * tmfwm_embed_px with one watermark tile per frame (added within ABI 10; the version number is
 * unchanged and existing entry points keep their behaviour): frame f is embedded with the
 * (height/block) x (width/block) tile at wm_tiles + f * tile_stride.  tile_stride = 0 is one tile
 * shared by every frame: exactly tmfwm_embed_px, which is this call with stride 0.  Any other
 * stride must be >= (height/block)*(width/block) (padded tiles are allowed; a smaller or
 * negative stride returns TMFWM_ERR_INVALID).  With TMFWM_MEM_HOST the n_frames tiles are
 * staged in one copy.  With TMFWM_MEM_DEVICE `out` must not overlap `rgb` nor the tiles' whole
 * span (n_frames - 1) * tile_stride + one tile.  Everything else -- pixel layouts, the frame
 * strides (one stride for 3 -> 3), block sizes, routes, *n_lapack_blocks -- as tmfwm_embed_px.
 * Extract takes no tile and has no counterpart.
 */
int tmfwm_embed_tiles(const uint8_t *rgb, int32_t in_pixel_bytes, int64_t in_frame_stride, int64_t n_frames, int32_t height,
                      int32_t width, const uint8_t *wm_tiles, int64_t tile_stride, int32_t block, double alpha, uint8_t *out,
                      int32_t out_pixel_bytes, int64_t out_frame_stride, int32_t mem_kind, void *hip_stream, int32_t route,
                      int64_t *n_lapack_blocks);

/*
 * Ragged batches (added within ABI 10; the version number is unchanged and existing entry points
 * keep their behaviour): n_frames frames of mixed sizes, each with its own buffers and its own
 * tile, embedded or extracted by one set of launches.  Every frame's bytes are exactly what
 * tmfwm_embed_route / tmfwm_extract_route give for that frame alone.
 *
 * One descriptor per frame.  The descriptor array itself is always host memory, whatever
 * mem_kind says about the pointers inside it; the library copies it before it returns, so the
 * caller may free or reuse it at once (also after an asynchronous TMFWM_MEM_DEVICE call).
 * Pixels are 3 bytes (TMFWM_PIX_RGB; the keyed *_ragged_px calls below take 4 as well), rows
 * packed: height x width x 3 bytes per image; the tile
 * is (height/block) x (width/block) bytes, packed.  A frame with height < block or
 * width < block has no block: embed writes its colour round trip, extract writes nothing for
 * it.  A frame with height == 0 or width == 0 is skipped (its pointers are not looked at).
 */
typedef struct {
    const uint8_t *rgb;      /* height x width x 3, packed rows */
    uint8_t *out;            /* same shape */
    const uint8_t *wm_tile;  /* (height/block) x (width/block), packed */
    int32_t height, width;
} tmfwm_embed_frame;

typedef struct {
    const uint8_t *wm_rgb, *orig_rgb;  /* both height x width x 3 */
    uint8_t *out_tile;                 /* (height/block) x (width/block) */
    int32_t height, width;
} tmfwm_extract_frame;

/*
 * Embed a ragged batch.  TMFWM_MEM_HOST: the frames are staged into one device allocation, the
 * results copied back, and the call returns when they have landed (tmfwm_embed's contract).
 * TMFWM_MEM_DEVICE: asynchronous on `hip_stream` unless n_lapack_blocks is given; every `out`
 * must be disjoint from every `rgb` and `wm_tile` of the call and from every other `out`
 * (TMFWM_ERR_INVALID otherwise; inputs may share memory).  Routes: TMFWM_ROUTE_HYBRID and
 * TMFWM_ROUTE_REFERENCE; this call and the other ragged calls here do not take the rank-1 routes
 * (TMFWM_ROUTE_RANK1 and TMFWM_ROUTE_RANK1_REFERENCE return TMFWM_ERR_UNSUPPORTED;
 * tmfwm_embed_ragged_rank1 and tmfwm_embed_key_ragged_rank1 below do).
 * *n_lapack_blocks (optional) receives the dgesdd-route blocks of all frames together; a dbdsqr
 * that does not converge fails a synchronising call as it does tmfwm_embed_ex.  The strip pass
 * runs every block to the end (no list pass): tmfwm_last_list_pass_blocks() reports 0.
 * All arguments are checked before the device is touched.
 */
int tmfwm_embed_ragged(const tmfwm_embed_frame *frames, int64_t n_frames, int32_t block, double alpha, int32_t mem_kind,
                       void *hip_stream, int32_t route, int64_t *n_lapack_blocks);

/* Extract a ragged batch: frame i's tile from its watermarked and original image (one size per
 * pair).  Memory kinds, routes, the count and the checks as tmfwm_embed_ragged; every `out_tile`
 * must be disjoint from the call's inputs and from every other `out_tile`; alpha must be finite
 * and non-zero. */
int tmfwm_extract_ragged(const tmfwm_extract_frame *frames, int64_t n_frames, int32_t block, double alpha, int32_t mem_kind,
                         void *hip_stream, int32_t route, int64_t *n_lapack_blocks);

/*
 * Keyed extraction over ragged batches (added within ABI 10; the version number is unchanged and
 * existing entry points keep their behaviour): the key maps and the keyed extracts of n_frames
 * frames of mixed sizes by one set of launches, so a verifier that stores keys instead of
 * originals takes uploads of any sizes through one call.  Frame i's key bits are exactly
 * tmfwm_sigma1_map's on that frame alone, and its tile bytes exactly tmfwm_extract_keyed's on
 * that frame alone with its key -- hence tmfwm_extract_route's with the original.  A key entry
 * that is not finite gives byte 0.
 *
 * Descriptors, pixel layout and frames without work as the ragged block above: the descriptor
 * array is host memory and is copied before the call returns; a frame with height < block or
 * width < block has no block, nothing is written for it and its key, out_key and out_tile
 * pointers are not looked at; a frame with height == 0 or width == 0 is skipped entirely.  A key
 * is (height/block) x (width/block) float32, packed, and must be 4-byte aligned
 * (TMFWM_ERR_INVALID otherwise, naming the frame).
 */
typedef struct {
    const uint8_t *rgb;   /* height x width x 3, packed rows: the original */
    float *out_key;       /* (height/block) x (width/block) float32, packed */
    int32_t height, width;
} tmfwm_key_frame;        /* 24 bytes */

typedef struct {
    const uint8_t *wm_rgb;  /* height x width x 3: the watermarked frame */
    const float *key;       /* (height/block) x (width/block) float32: sigma1 map of its original */
    uint8_t *out_tile;      /* (height/block) x (width/block) */
    int32_t height, width;
} tmfwm_keyed_frame;      /* 32 bytes */

/*
 * Memory kinds, routes, *n_lapack_blocks, the non-convergence report and the checks as
 * tmfwm_embed_ragged: TMFWM_MEM_HOST stages every piece into one device allocation and returns
 * when the results have landed; TMFWM_MEM_DEVICE is asynchronous on `hip_stream` unless
 * n_lapack_blocks is given.  TMFWM_ROUTE_HYBRID certifies the enclosure in the strip pass and
 * sends the undecided blocks straight to the dgesdd route (no list pass:
 * tmfwm_last_list_pass_blocks() reports 0), TMFWM_ROUTE_REFERENCE sends every block there; the
 * rank-1 routes return TMFWM_ERR_UNSUPPORTED.  With TMFWM_MEM_DEVICE every `out_key` /
 * `out_tile` must be disjoint from every input of the call and from every other output
 * (TMFWM_ERR_INVALID otherwise).  Inputs may share memory: many frames may point at one key (one
 * original, many watermarked copies), the ragged form of tmfwm_extract_keyed's key_stride = 0.
 * The map takes no alpha; the extract's must be finite and non-zero.
 */
int tmfwm_sigma1_map_ragged(const tmfwm_key_frame *frames, int64_t n_frames, int32_t block, int32_t mem_kind,
                            void *hip_stream, int32_t route, int64_t *n_lapack_blocks);
int tmfwm_extract_keyed_ragged(const tmfwm_keyed_frame *frames, int64_t n_frames, int32_t block, double alpha,
                               int32_t mem_kind, void *hip_stream, int32_t route, int64_t *n_lapack_blocks);

/*
 * The same two calls with a pixel layout (added within ABI 10): one layout per call, every image
 * height x width x pixel_bytes, rows packed (TMFWM_PIX_RGB or TMFWM_PIX_RGBX; anything else is
 * TMFWM_ERR_INVALID).  The descriptors are unchanged.  4-byte images are read where they lie, as
 * tmfwm_sigma1_map_px reads them (dwords for an image whose pointer is 4-byte aligned, bytes
 * otherwise); key bits and tile bytes are those of the 3-byte call on the same R, G, B values.
 * With pixel_bytes == 3 each call is its sibling above.
 */
int tmfwm_sigma1_map_ragged_px(const tmfwm_key_frame *frames, int64_t n_frames, int32_t block, int32_t pixel_bytes,
                               int32_t mem_kind, void *hip_stream, int32_t route, int64_t *n_lapack_blocks);
int tmfwm_extract_keyed_ragged_px(const tmfwm_keyed_frame *frames, int64_t n_frames, int32_t block, double alpha,
                                  int32_t pixel_bytes, int32_t mem_kind, void *hip_stream, int32_t route,
                                  int64_t *n_lapack_blocks);

/*
 * Embed that also returns the extraction key (added within ABI 10; the version number is
 * unchanged and existing entry points keep their behaviour): the enrolment side of keyed
 * extraction in one call.  `out` receives exactly tmfwm_embed_route's bytes (per-frame tiles as
 * tmfwm_embed_tiles: frame f's tile at wm_tiles + f * tile_stride, 0 = one shared tile) and
 * out_key exactly tmfwm_sigma1_map's key of the ORIGINAL frames `rgb` -- the key that
 * tmfwm_extract_keyed takes with the frames in `out`.  The key depends on neither alpha nor the
 * tiles nor the route.
 *
 * On TMFWM_ROUTE_HYBRID and TMFWM_ROUTE_REFERENCE the key comes out of the embed passes: the embed
 * kernels already hold sigma_1 of every block and store f32(sigma_1) where its certified
 * enclosure is one float; a block where it is not (about 2^-20 of them) joins the dgesdd-route
 * blocks, whose pass stores its own S[0], so *n_lapack_blocks may exceed tmfwm_embed_route's by
 * those blocks.  On the rank-1 routes the call runs tmfwm_embed_route's passes and then
 * tmfwm_sigma1_map's on the same stream, and *n_lapack_blocks and
 * tmfwm_last_list_pass_blocks() are the sums over both.
 *
 * key_stride: bytes between consecutive frames' keys, a multiple of 4 and
 * >= (height/block)*(width/block)*4 (TMFWM_ERR_INVALID otherwise); ignored for n_frames == 1.
 * Bytes of a padded stride outside the keys are not written.  out_key must be 4-byte aligned and,
 * with TMFWM_MEM_DEVICE, disjoint from rgb, wm_tiles and out (TMFWM_ERR_INVALID otherwise).  A
 * frame size without a block gets its colour round trip and no key entry (out_key is not looked
 * at).  Memory kinds (TMFWM_MEM_HOST stages the keys back with the pixels), chunking, the count
 * and the non-convergence report as tmfwm_embed_route.  Pixels are 3 bytes (TMFWM_PIX_RGB);
 * tmfwm_embed_key_px takes a pixel layout per side.
 */
int tmfwm_embed_key(const uint8_t *rgb, int64_t n_frames, int32_t height, int32_t width, int64_t frame_stride,
                    const uint8_t *wm_tiles, int64_t tile_stride, int32_t block, double alpha, uint8_t *out,
                    float *out_key, int64_t key_stride, int32_t mem_kind, void *hip_stream, int32_t route,
                    int64_t *n_lapack_blocks);

/*
 * tmfwm_embed_key with a pixel layout per side (added within ABI 10): the arguments of
 * tmfwm_embed_tiles, plus out_key and key_stride as tmfwm_embed_key has them.  `out` receives
 * tmfwm_embed_tiles' bytes (pad 255 on 4-byte output) and out_key tmfwm_sigma1_map's key of the
 * R, G, B values in `rgb`.  The call writes pixels, so 4-byte frames are converted on the device
 * as in tmfwm_embed_tiles, and the key comes out of the embed passes over the packed frames.
 * 3 -> 3 is tmfwm_embed_key (one frame stride for both).  key_stride, out_key's alignment and
 * pixel_bytes are checked before the device is touched.
 */
int tmfwm_embed_key_px(const uint8_t *rgb, int32_t in_pixel_bytes, int64_t in_frame_stride, int64_t n_frames, int32_t height,
                       int32_t width, const uint8_t *wm_tiles, int64_t tile_stride, int32_t block, double alpha, uint8_t *out,
                       int32_t out_pixel_bytes, int64_t out_frame_stride, float *out_key, int64_t key_stride,
                       int32_t mem_kind, void *hip_stream, int32_t route, int64_t *n_lapack_blocks);

/*
 * The same over a ragged batch: tmfwm_embed_ragged's frames, each with a key output.  Frame i's
 * `out` bytes are tmfwm_embed_ragged's and its key bits tmfwm_sigma1_map_ragged's.  Descriptors,
 * memory kinds, routes (TMFWM_ROUTE_HYBRID and TMFWM_ROUTE_REFERENCE), the count and the checks as
 * tmfwm_embed_ragged; every `out` and every `out_key` must be disjoint from every input of the
 * call and from every other output (TMFWM_ERR_INVALID otherwise), and every out_key 4-byte
 * aligned.  A frame without a block gets its colour round trip; its out_key is not looked at.
 */
typedef struct {
    const uint8_t *rgb;      /* height x width x 3, packed rows: the original */
    uint8_t *out;            /* same shape: the watermarked frame */
    const uint8_t *wm_tile;  /* (height/block) x (width/block), packed */
    float *out_key;          /* (height/block) x (width/block) float32, packed */
    int32_t height, width;
} tmfwm_embed_key_frame;     /* 40 bytes */
int tmfwm_embed_key_ragged(const tmfwm_embed_key_frame *frames, int64_t n_frames, int32_t block, double alpha,
                           int32_t mem_kind, void *hip_stream, int32_t route, int64_t *n_lapack_blocks);

/*
 * The ragged embed on every route (added within ABI 10; the version number is unchanged, and
 * tmfwm_embed_ragged / tmfwm_embed_key_ragged keep refusing the rank-1 routes).  Descriptors,
 * memory kinds, the overlap checks, frames without a block, zero-area frames, the count, the
 * non-convergence report and "all arguments checked before the device is touched" are
 * tmfwm_embed_ragged's.  TMFWM_ROUTE_HYBRID and TMFWM_ROUTE_REFERENCE are that call, unchanged.
 * TMFWM_ROUTE_RANK1 and TMFWM_ROUTE_RANK1_REFERENCE run the rank-1 pre-pass over every frame's
 * blocks in one launch (any block size 4..16 even); the blocks it leaves go to one list pass on
 * the hybrid route (TMFWM_ROUTE_RANK1) or straight to the dgesdd route
 * (TMFWM_ROUTE_RANK1_REFERENCE).  Frame i's bytes are tmfwm_embed_route's on that frame alone on
 * the same route -- the reference route's on every route.  *n_lapack_blocks is the sum over the
 * frames, and tmfwm_last_list_pass_blocks() reports what the pre-pass left to the list pass on
 * TMFWM_ROUTE_RANK1.
 */
int tmfwm_embed_ragged_rank1(const tmfwm_embed_frame *frames, int64_t n_frames, int32_t block, double alpha, int32_t mem_kind,
                             void *hip_stream, int32_t route, int64_t *n_lapack_blocks);

/*
 * tmfwm_embed_key_ragged on every route.  TMFWM_ROUTE_HYBRID and TMFWM_ROUTE_REFERENCE are that
 * call, unchanged.  On the rank-1 routes the call is composed, as tmfwm_embed_key is there:
 * tmfwm_embed_ragged_rank1's passes, then tmfwm_sigma1_map_ragged's on the same stream over the
 * same buffers (TMFWM_MEM_HOST: over the one staged copy).  Frame i's `out` bytes are
 * tmfwm_embed_ragged_rank1's, its key bits tmfwm_sigma1_map_ragged's, and the counts are the sums
 * over both.
 */
int tmfwm_embed_key_ragged_rank1(const tmfwm_embed_key_frame *frames, int64_t n_frames, int32_t block, double alpha,
                                 int32_t mem_kind, void *hip_stream, int32_t route, int64_t *n_lapack_blocks);

/*
 * The ragged calls with one alpha per frame (added within ABI 10; the version number is unchanged
 * and the calls above keep their signatures and behaviour): uploads of several sessions, each
 * with its own strength setting, or one cover at several strengths, in one set of launches.
 * `alphas` is n_frames doubles in host memory whatever mem_kind says, copied with the descriptors
 * before the call returns; NULL with n_frames > 0 is TMFWM_ERR_INVALID.  Every entry is checked
 * before the device is touched, whether or not its frame has a block -- finite for the embeds,
 * finite and non-zero for the extracts -- and the message names the frame index.
 *
 * Frame i's output bytes are those of the uniform call on that frame alone with alpha = alphas[i]
 * (the key bits likewise; they do not depend on alpha), hence tmfwm_embed_route's /
 * tmfwm_extract_route's / tmfwm_extract_keyed's on that frame; the extracts divide by
 * f32(alphas[i]).  Descriptors, memory kinds, the overlap rules, frames without a block, chunking,
 * the count, tmfwm_last_list_pass_blocks() and the non-convergence report are the uniform
 * siblings'.  The embeds take all four routes, as tmfwm_embed_ragged_rank1 /
 * tmfwm_embed_key_ragged_rank1 do (the key call composed on the rank-1 routes as there); the
 * extracts take TMFWM_ROUTE_HYBRID and TMFWM_ROUTE_REFERENCE; the keyed extract takes 3- or 4-byte
 * pixels as tmfwm_extract_keyed_ragged_px does.
 */
int tmfwm_embed_ragged_alphas(const tmfwm_embed_frame *frames, const double *alphas, int64_t n_frames, int32_t block,
                              int32_t mem_kind, void *hip_stream, int32_t route, int64_t *n_lapack_blocks);
int tmfwm_embed_key_ragged_alphas(const tmfwm_embed_key_frame *frames, const double *alphas, int64_t n_frames, int32_t block,
                                  int32_t mem_kind, void *hip_stream, int32_t route, int64_t *n_lapack_blocks);
int tmfwm_extract_ragged_alphas(const tmfwm_extract_frame *frames, const double *alphas, int64_t n_frames, int32_t block,
                                int32_t mem_kind, void *hip_stream, int32_t route, int64_t *n_lapack_blocks);
int tmfwm_extract_keyed_ragged_alphas(const tmfwm_keyed_frame *frames, const double *alphas, int64_t n_frames, int32_t block,
                                      int32_t pixel_bytes, int32_t mem_kind, void *hip_stream, int32_t route,
                                      int64_t *n_lapack_blocks);

/* tmfwm_extract_route with a pixel layout and frame stride per input image (ABI 8). */
int tmfwm_extract_px(const uint8_t *wm_rgb, int32_t wm_pixel_bytes, int64_t wm_frame_stride, const uint8_t *orig_rgb,
                     int32_t orig_pixel_bytes, int64_t orig_frame_stride, int64_t n_frames, int32_t height, int32_t width,
                     int32_t block, double alpha, uint8_t *out_tiles, int32_t mem_kind, void *hip_stream, int32_t route,
                     int64_t *n_lapack_blocks);

/*
 * Multi-GPU embed / extract for callers without torch.distributed (one process drives
 * several devices).  Host memory only: rgb / out (wm_rgb / orig_rgb / out_tiles) are host
 * buffers laid out as for tmfwm_embed / tmfwm_extract, and the call returns when every
 * result is back.  The n_frames frames are split into n_shards contiguous shards (sizes
 * differ by at most one, shard s gets frames [s*n/k + min(s, n%k), ...)), shard s runs on
 * HIP device devices[s] (devices = NULL: device s; n_shards <= 0 with devices = NULL: every
 * visible device) on its own host thread and streams, in passes through two device slots of ~1 GiB of
 * frames.  The watermark tile is uploaded to devices[0] and broadcast to every other
 * device of the set with RCCL (ncclBroadcast over xGMI; librccl.so.1 is loaded on first
 * use).  Shards naming the same device share its tile (logical shards).  Replaces the
 * app's per-image loop (internal_pages/embed_watermark_page.py:492-558) for a batch; the
 * per-frame arithmetic is tmfwm_embed's.  *n_lapack_blocks (optional) sums the shards'
 * dgesdd-route blocks.  The calling thread's current HIP device is preserved.
 */
int tmfwm_embed_multi(const uint8_t *rgb, int64_t n_frames, int32_t height, int32_t width, int64_t frame_stride,
                      const uint8_t *wm_tile, int32_t block, double alpha, uint8_t *out, const int32_t *devices,
                      int32_t n_shards, int64_t *n_lapack_blocks);

int tmfwm_extract_multi(const uint8_t *wm_rgb, const uint8_t *orig_rgb, int64_t n_frames, int32_t height, int32_t width,
                        int64_t frame_stride, int32_t block, double alpha, uint8_t *out_tiles, const int32_t *devices,
                        int32_t n_shards, int64_t *n_lapack_blocks);

/* The multi-GPU calls with an explicit SVD route (ABI 8; TMFWM_ROUTE_*, as tmfwm_embed_route):
 * tmfwm_embed_multi / tmfwm_extract_multi are these with TMFWM_ROUTE_HYBRID. */
int tmfwm_embed_multi_route(const uint8_t *rgb, int64_t n_frames, int32_t height, int32_t width, int64_t frame_stride,
                            const uint8_t *wm_tile, int32_t block, double alpha, uint8_t *out, const int32_t *devices,
                            int32_t n_shards, int32_t route, int64_t *n_lapack_blocks);
int tmfwm_extract_multi_route(const uint8_t *wm_rgb, const uint8_t *orig_rgb, int64_t n_frames, int32_t height, int32_t width,
                              int64_t frame_stride, int32_t block, double alpha, uint8_t *out_tiles, const int32_t *devices,
                              int32_t n_shards, int32_t route, int64_t *n_lapack_blocks);

/*
 * tmfwm_embed_multi_route with one watermark tile per frame (added within ABI 10): frame f's
 * tile is the host buffer wm_tiles + f * tile_stride (tile_stride >= (height/block)*(width/block);
 * 0 is the shared tile of tmfwm_embed_multi_route, broadcast as described above).  In per-frame
 * mode nothing is broadcast and librccl is not needed: every pass of a shard uploads the tiles
 * of its own frames with those frames (1/192 of their bytes at block = 8), so a device only
 * ever receives the tiles of the frames it embeds.
 */
int tmfwm_embed_multi_tiles(const uint8_t *rgb, int64_t n_frames, int32_t height, int32_t width, int64_t frame_stride,
                            const uint8_t *wm_tiles, int64_t tile_stride, int32_t block, double alpha, uint8_t *out,
                            const int32_t *devices, int32_t n_shards, int32_t route, int64_t *n_lapack_blocks);

/* Frees the device staging buffers the multi-GPU calls keep between calls (at most four free
 * buffers per device are kept; ABI 9).  Returns the number of buffers freed. */
int tmfwm_release_cached_buffers(void);

/* rgb_to_ycbcr (watermarking.py:23): npix RGB uint8 pixels -> npix x 3 float32 (Y, Cb+0.5, Cr+0.5). */
int tmfwm_rgb_to_ycbcr(const uint8_t *rgb, int64_t npix, float *ycc, int32_t mem_kind, void *hip_stream);

/* ycbcr_to_rgb (watermarking.py:53): npix x 3 float32 -> RGB uint8 (clip, *255, truncate). */
int tmfwm_ycbcr_to_rgb(const float *ycc, int64_t npix, uint8_t *rgb, int32_t mem_kind, void *hip_stream);

/* Element types of the typed helper entry points below. */
#define TMFWM_DT_F16 1
#define TMFWM_DT_F32 2
#define TMFWM_DT_F64 3

/* rgb_to_ycbcr (watermarking.py:23-50) of a non-uint8 input: rgb holds npix x 3 float32
 * values on the 0..255 scale, i.e. the input after the reference's own cast
 * np.array(img, dtype=np.float32) (:29), which stays with the caller; the "/ 255.0" and
 * the rest run here.  For integral values it equals tmfwm_rgb_to_ycbcr. */
int tmfwm_rgb_to_ycbcr_f32(const float *rgb, int64_t npix, float *ycc, int32_t mem_kind, void *hip_stream);

/* ycbcr_to_rgb (watermarking.py:53-73) of an npix x 3 array of element type dtype
 * (TMFWM_DT_F16 = IEEE binary16 / numpy float16, _F32, _F64).  The reference computes in the
 * input's own type (:55 img.copy()): "-= 0.5", the stored dot product, clip and "* 255" are
 * rounded to that type, so a float64 input is not the float32 result of its cast.
 * TMFWM_DT_F32 is tmfwm_ycbcr_to_rgb.  Non-finite inputs have no defined uint8 (neither in
 * the reference: NaN -> uint8 is undefined in C and numpy). */
int tmfwm_ycbcr_to_rgb_typed(const void *ycc, int32_t dtype, int64_t npix, uint8_t *rgb, int32_t mem_kind,
                             void *hip_stream);

/* apply_dct_to_block / apply_idct_to_block (watermarking.py:76, :81) on n_blocks
 * contiguous row-major block x block float32 blocks, in place. */
int tmfwm_dct2d_blocks(float *blocks, int64_t n_blocks, int32_t block, int32_t inverse, int32_t mem_kind,
                       void *hip_stream);

/* np.linalg.svd(D) as the reference consumes it (watermarking.py:195): U, S
 * (descending), Vt in float32 for n_blocks blocks.  sweeps (optional, may be
 * NULL) receives the Jacobi sweeps per block: f64 sweeps | (f32 sweeps << 8)
 * (0 for an all-zero block). */
int tmfwm_svd_blocks(const float *D, int64_t n_blocks, int32_t block, float *U, float *S, float *Vt, int32_t *sweeps,
                     int32_t mem_kind, void *hip_stream);

/* np.linalg.svd(D) on the dgesdd route (the reference's own arithmetic, restated for the
 * GPU): U, S (descending), Vt in float32 for n_blocks row-major blocks.  want_vectors = 0
 * computes S only (U and Vt may be NULL).  Synchronises `hip_stream`; a block on which
 * dbdsqr does not converge returns TMFWM_ERR_INVALID. */
int tmfwm_lapack_svd_blocks(const float *D, int64_t n_blocks, int32_t block, float *U, float *S, float *Vt,
                            int32_t want_vectors, int32_t mem_kind, void *hip_stream);

/* OpenBLAS dnrm2 as LAPACK's dlarfg sees it (x87 extended arithmetic, emulated): out[v]
 * = nrm2 of n elements, stride inc, of vector v (vectors n*inc doubles apart). */
int tmfwm_lapack_nrm2(const double *x, int64_t n_vectors, int32_t n, int32_t inc, double *out, int32_t mem_kind,
                      void *hip_stream);

/* Synthetic frames generated in device memory (bench inputs):
 * out[f*frame_bytes + i] = splitmix64(seed ^ ((frame0+f) << 40) ^ i) & 0xFF. */
int tmfwm_synth_frames(uint64_t seed, int64_t frame0, int64_t n_frames, int64_t frame_bytes, uint8_t *out,
                       void *hip_stream);

/*
 * Watermark preparation: replaces resize_watermark() (watermarking.py:86-132)
 * after its PNG decode and convert("L") (:98-103), which stay with the caller.
 * wm: wm_height x wm_width 8-bit grey pixels.  tile: tile_height x tile_width.
 * preserve_ratio = 0: Pillow 12.2.0 Image.resize((tile_width, tile_height),
 * LANCZOS) (:127-130).  preserve_ratio != 0: LANCZOS to (int(w*r), int(h*r)),
 * r = min(tile_width/w, tile_height/h), pasted centred on a white (255) canvas
 * (:105-123).  Bytes equal Pillow's (fixed-point Resample.c).  Synchronises
 * `hip_stream` before returning (the resample tables are built on the host).
 * Empty sizes return TMFWM_ERR_INVALID (PIL raises ValueError there).
 */
int tmfwm_prepare_tile(const uint8_t *wm, int32_t wm_height, int32_t wm_width, int32_t tile_height, int32_t tile_width,
                       int32_t preserve_ratio, uint8_t *tile, int32_t mem_kind, void *hip_stream);

/*
 * tmfwm_prepare_tile for a batch (added within ABI 10): n_wm grey watermarks of one size
 * (text_to_qrcode always renders 300 x 300), wm_stride bytes apart (>= wm_height*wm_width), to
 * n_wm tiles tile_stride bytes apart (>= tile_height*tile_width; the bytes between padded tiles
 * are not written).  One set of resample tables is built and uploaded for the whole batch and
 * each resample pass is one launch over all the watermarks (groups of 1024), the white canvas
 * and centred paste of preserve_ratio included; a tile of the watermark's own size is a copy.
 * There is no host round trip per tile: the stream is synchronised once, at the end.  Every
 * tile's bytes are tmfwm_prepare_tile's, which is this call with n_wm = 1.
 */
int tmfwm_prepare_tiles(const uint8_t *wm, int64_t n_wm, int32_t wm_height, int32_t wm_width, int64_t wm_stride,
                        int32_t tile_height, int32_t tile_width, int32_t preserve_ratio, uint8_t *tiles, int64_t tile_stride,
                        int32_t mem_kind, void *hip_stream);

/*
 * Ragged tile preparation (added within ABI 10; the version number is unchanged and the two calls
 * above keep their behaviour, their synchronisation included): n_jobs jobs, each with its own
 * watermark and its own tile, both of any size, resampled by one set of launches.  Every tile's
 * bytes are tmfwm_prepare_tile's for that job alone; preserve_ratio is one flag for the call.
 *
 * The descriptor array is host memory whatever mem_kind says about the pointers inside it, and
 * the library copies it before it returns.  Each distinct (input size, output size) resample axis
 * of the call is built once and shared by the jobs and the two directions that use it; all tables
 * and the job table go to the device in one copy.  TMFWM_MEM_DEVICE: the call enqueues on
 * `hip_stream` and returns without synchronising; every `tile` must be disjoint from every `wm`
 * of the call and from every other `tile` (TMFWM_ERR_INVALID otherwise), while watermarks may
 * share memory (one watermark for many sizes).  TMFWM_MEM_HOST: watermarks and tiles are staged,
 * the tiles copied back, and the call returns when they have landed.
 *
 * All arguments are checked before the device is touched, no job is skipped, and nothing is
 * written when a job is refused: a size <= 0 or an empty resized size under preserve_ratio
 * ("job i" in the message; tmfwm_prepare_tile refuses the same inputs) and a NULL pointer return
 * TMFWM_ERR_INVALID.  n_jobs == 0 does nothing.
 */
typedef struct {
    const uint8_t *wm;    /* wm_height x wm_width grey bytes, packed rows */
    uint8_t *tile;        /* tile_height x tile_width, packed */
    int32_t wm_height, wm_width, tile_height, tile_width;
} tmfwm_tile_job;         /* 32 bytes */

int tmfwm_prepare_tiles_ragged(const tmfwm_tile_job *jobs, int64_t n_jobs, int32_t preserve_ratio, int32_t mem_kind,
                               void *hip_stream);

/*
 * The watermark's payload, host-side C++ (no GPU, no torch): the QR codec
 * and AES-CBC the app wraps around embed / extract.  The reference builds the watermark with
 * modules/encryption.py:8-40 (encrypt_watermark: random 16-byte IV + AES-CBC of the
 * PKCS#7-padded text) and modules/qrcode_generator.py:10-44 (text_to_qrcode: base64 text,
 * python-qrcode ERROR_CORRECT_H, version >= 1 fitted, box 10, border 4, 300 x 300), and reads
 * it back with qrcode_to_text (:47-76, pyzbar) and decrypt_watermark (encryption.py:43-68,
 * pycryptodome) at internal_pages/extract_watermark_page.py:356-364.
 *
 * tmfwm_qr_encode: data -> size x size modules (1 = dark, row-major) of the smallest version
 * >= min_version (1..10) that fits at ec_level (0 L, 1 M, 2 Q, 3 H), segmented and masked as
 * python-qrcode does (mask = -1: lowest penalty; 0..7 forces one).  *size_out = 17 + 4 v
 * (also on a too-small buffer, TMFWM_ERR_INVALID).  Data beyond version 10: TMFWM_ERR_UNSUPPORTED.
 */
int tmfwm_qr_encode(const uint8_t *data, int32_t len, int32_t ec_level, int32_t min_version, int32_t mask, uint8_t *modules,
                    int32_t capacity, int32_t *size_out);

/* tmfwm_qr_decode: an upright QR symbol (versions 1..10) in an 8-bit grey image (dark =
 * low), e.g. an extracted watermark tile, -> its payload bytes (numeric, alphanumeric and
 * byte segments, Reed-Solomon corrected).  TMFWM_ERR_NODATA when no symbol decodes;
 * *len_out = payload length (also when capacity is too small: TMFWM_ERR_INVALID). */
int tmfwm_qr_decode(const uint8_t *gray, int32_t height, int32_t width, int64_t row_stride, uint8_t *out, int32_t capacity,
                    int32_t *len_out);

/* tmfwm_qr_decode over n_tiles back-to-back height x width tiles (tmfwm_extract's output
 * layout), on host threads: payload of tile i at out + i*capacity, lens[i] = its length or
 * -1 when the tile holds no decodable symbol (or it exceeds capacity). */
int tmfwm_qr_decode_batch(const uint8_t *tiles, int64_t n_tiles, int32_t height, int32_t width, uint8_t *out, int32_t capacity,
                          int32_t *lens);

/* AES-CBC (FIPS-197, SP 800-38A) with a 16 / 24 / 32-byte key and a 16-byte IV over len bytes
 * (a multiple of 16; padding is the caller's: PKCS#7 in the app).  out may equal in. */
int tmfwm_aes_cbc_encrypt(const uint8_t *key, int32_t key_len, const uint8_t *iv, const uint8_t *in, int64_t len,
                          uint8_t *out);
int tmfwm_aes_cbc_decrypt(const uint8_t *key, int32_t key_len, const uint8_t *iv, const uint8_t *in, int64_t len,
                          uint8_t *out);

#ifdef __cplusplus
}
#endif

#endif /* TMFWM_H */
