// The launch geometry of the depthwise 7x7 channels-last convolution (csrc/dwconv.hip): uc_dwconv7x7_nhwc and its weight gradient.
//
// Forward.  A workgroup computes one tile of tile_h x tile_w output pixels for one chunk of c8 8-channel vectors.  It stages the tile
// plus its 3-pixel halo, (tile_h + 6) x (tile_w + 6) pixels, in LDS in the storage dtype (zeros outside the map and beyond C), and the 49
// weight vectors of the chunk in fp32.  A work item owns one 8-channel vector and a run of UC_DW_RUN = 4 horizontally adjacent outputs:
// per tap row it reads 4 + 6 vectors from LDS and uses each for up to four outputs.  The full tile is 16 x 16: every pixel of the map is
// staged by (22 * 22) / (16 * 16) = 1.89 workgroups (the halo overhead; the re-reads are neighbours' tiles and hit the L2).  A map smaller
// than the tile shrinks the tile (tile_w rounded up to the run) and widens the chunk instead, as far as 32 vectors and the LDS budget go.
// A pixel's LDS stride is c8 | 1 vectors (odd), so the lanes of consecutive runs do not start on the same banks.
//
// Weight gradient.  A workgroup owns one channel chunk and every `partials`-th unit (image, tile) of the map; a work item owns
// (vector, tap row ky, row group) and accumulates the 7 taps of its row (and, for ky == 0, the bias gradient) over its units in
// registers, rows and columns ascending; the row groups are then merged in ascending order through LDS and the workgroup writes ONE
// partial [50][C-chunk] to the caller's workspace [partials][50][C]; a second kernel adds the partials in ascending order.
//
// Host-only, header-only and pure: no HIP header, no global state, no knob, so the system C++ compiler builds it
// (tests/dwconv_plan_driver.cpp).  The entry points validate, call their plan once and carry it out; the kernels decode a workgroup
// index with the functions below, so the driver walks exactly what the device walks.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define UC_DW_HD __host__ __device__
#else
#define UC_DW_HD
#endif

static constexpr int UC_DW_DT_F32 = 0, UC_DW_DT_BF16 = 1, UC_DW_DT_F16 = 2;    // UC_F32 / UC_BF16 / UC_F16 of include/uc_hip.h
static constexpr int UC_DW_TAPS = 49, UC_DW_RADIUS = 3;
static constexpr int UC_DW_RUN = 4;                 // outputs along a row per work item
static constexpr int UC_DW_TILE = 16;               // forward: full tile edge
static constexpr int UC_DW_WGRAD_TILE_H = 8;        // weight gradient: full tile height (its width is UC_DW_TILE)
static constexpr int UC_DW_MAX_THREADS = 256;
static constexpr int UC_DW_MAX_C8 = 32;             // widest channel chunk, in 8-channel vectors
static constexpr int UC_DW_LDS_BUDGET = 65536;      // bytes of LDS one workgroup may ask for
static constexpr int UC_DW_WGRAD_WORK = 32768;     // weight gradient: partials = min(units, WORK / C), about a thousand workgroups, whatever the dtype
static constexpr int UC_DW_WS_ROWS = UC_DW_TAPS + 1;    // rows of one partial: 49 taps, then the bias gradient

static inline int uc_dw_vec_bytes(int dtype) { return dtype == UC_DW_DT_F32 ? 32 : 16; }
static inline int uc_dw_min(int a, int b) { return a < b ? a : b; }
static inline int uc_dw_ceil(int a, int b) { return (a + b - 1) / b; }

struct DwconvPlan {
    int tile_h, tile_w;         // output pixels of a tile (tile_w: a multiple of UC_DW_RUN)
    int c8;                     // 8-channel vectors of a channel chunk
    int pix_stride;             // LDS stride of one staged pixel, in vectors: c8 | 1
    int chunks, tiles_y, tiles_x;
    int items;                  // work items of a tile: c8 * tile_h * tile_w / UC_DW_RUN  (<= threads)
    int threads;                // workgroup size: items rounded up to a wavefront
    int vec_bytes;              // bytes of an 8-channel vector in the storage dtype
    int lds_in_bytes, lds_w_bytes, lds_bytes;
    int64_t grid;               // B * chunks * tiles_y * tiles_x workgroups (x fastest, then y, chunk, image)
};

static inline int uc_dw_lds_in(int th, int tw, int c8, int vb) { return (th + 2 * UC_DW_RADIUS) * (tw + 2 * UC_DW_RADIUS) * (c8 | 1) * vb; }

// B, H, W, C > 0 and C % 8 == 0 (the entry point has checked).
static inline DwconvPlan uc_dwconv_plan(int dtype, int B, int H, int W, int C) {
    DwconvPlan p = {};
    const int C8 = C / 8;
    p.vec_bytes = uc_dw_vec_bytes(dtype);
    p.tile_h = uc_dw_min(H, UC_DW_TILE);
    p.tile_w = uc_dw_min(uc_dw_ceil(W, UC_DW_RUN) * UC_DW_RUN, UC_DW_TILE);
    const int per_c8 = p.tile_h * (p.tile_w / UC_DW_RUN);
    int c = uc_dw_min(C8, UC_DW_MAX_C8);
    while (c > 1 && (c * per_c8 > UC_DW_MAX_THREADS || uc_dw_lds_in(p.tile_h, p.tile_w, c, p.vec_bytes) + UC_DW_TAPS * c * 32 > UC_DW_LDS_BUDGET)) --c;
    p.chunks = uc_dw_ceil(C8, c);
    p.c8 = uc_dw_ceil(C8, p.chunks);        // even the chunks out (40 channels: 3 + 2 vectors, not 4 + 1)
    p.pix_stride = p.c8 | 1;
    p.tiles_y = uc_dw_ceil(H, p.tile_h);
    p.tiles_x = uc_dw_ceil(W, p.tile_w);
    p.items = p.c8 * per_c8;
    p.threads = uc_dw_ceil(p.items, 64) * 64;
    p.lds_in_bytes = uc_dw_lds_in(p.tile_h, p.tile_w, p.c8, p.vec_bytes);
    p.lds_w_bytes = UC_DW_TAPS * p.c8 * 32;
    p.lds_bytes = p.lds_in_bytes + p.lds_w_bytes;
    p.grid = (int64_t)B * p.chunks * p.tiles_y * p.tiles_x;
    return p;
}

struct DwconvBlock { int b, chunk, ty, tx; };
UC_DW_HD static inline DwconvBlock uc_dwconv_block(int tiles_x, int tiles_y, int chunks, int64_t block) {
    DwconvBlock k;
    k.tx = (int)(block % tiles_x); block /= tiles_x;
    k.ty = (int)(block % tiles_y); block /= tiles_y;
    k.chunk = (int)(block % chunks);
    k.b = (int)(block / chunks);
    return k;
}

// work item -> (vector of the chunk, run of the row, row of the tile)
struct DwconvItem { int c8, run, row; };
UC_DW_HD static inline DwconvItem uc_dwconv_item(int c8n, int tile_w, int item) {
    DwconvItem t;
    const int runs = tile_w / UC_DW_RUN;
    t.c8 = item % c8n; item /= c8n;
    t.run = item % runs;
    t.row = item / runs;
    return t;
}

struct DwconvWgradPlan {
    int tile_h, tile_w, c8, pix_stride, chunks, tiles_y, tiles_x;
    int row_groups;             // work items that share (vector, ky) and split the tile's rows: row = group, group + row_groups, ...
    int threads;                // 7 * c8 * row_groups rounded up to a wavefront
    int vec_bytes;
    int lds_x_bytes, lds_dy_bytes, lds_red_bytes, lds_bytes;
    int64_t units;              // B * tiles_y * tiles_x (x fastest, then y, image)
    int partials;               // workgroups per chunk = partial sums per output; workgroup q takes units q, q + partials, ...
    int merge_depth;            // additions that join partial sums: (row_groups - 1) + (partials - 1)
    int64_t ws_bytes;           // partials * 50 * C * 4
};

static inline int uc_dw_wgrad_lds(int th, int tw, int c8, int vb) {
    return uc_dw_lds_in(th, tw, c8, vb) + th * tw * (c8 | 1) * vb + UC_DW_WS_ROWS * c8 * 32;
}

static inline DwconvWgradPlan uc_dwconv_wgrad_plan(int dtype, int64_t B, int H, int W, int C) {
    DwconvWgradPlan p = {};
    const int C8 = C / 8;
    p.vec_bytes = uc_dw_vec_bytes(dtype);
    p.tile_h = uc_dw_min(H, UC_DW_WGRAD_TILE_H);
    p.tile_w = uc_dw_min(uc_dw_ceil(W, UC_DW_RUN) * UC_DW_RUN, UC_DW_TILE);
    p.row_groups = p.tile_h;
    int c = uc_dw_min(C8, UC_DW_MAX_C8);
    while (c > 1 && (7 * c * p.row_groups > UC_DW_MAX_THREADS || uc_dw_wgrad_lds(p.tile_h, p.tile_w, c, p.vec_bytes) > UC_DW_LDS_BUDGET)) --c;
    p.chunks = uc_dw_ceil(C8, c);
    p.c8 = uc_dw_ceil(C8, p.chunks);
    p.pix_stride = p.c8 | 1;
    p.tiles_y = uc_dw_ceil(H, p.tile_h);
    p.tiles_x = uc_dw_ceil(W, p.tile_w);
    p.threads = uc_dw_ceil(7 * p.c8 * p.row_groups, 64) * 64;
    p.lds_x_bytes = uc_dw_lds_in(p.tile_h, p.tile_w, p.c8, p.vec_bytes);
    p.lds_dy_bytes = p.tile_h * p.tile_w * p.pix_stride * p.vec_bytes;
    p.lds_red_bytes = UC_DW_WS_ROWS * p.c8 * 32;
    p.lds_bytes = p.lds_x_bytes + p.lds_dy_bytes + p.lds_red_bytes;
    p.units = B * p.tiles_y * p.tiles_x;
    const int64_t want = UC_DW_WGRAD_WORK / C > 0 ? UC_DW_WGRAD_WORK / C : 1;      // (tiles and C only: the workspace size does not depend on the dtype)
    p.partials = (int)(p.units < want ? p.units : want);
    p.merge_depth = (p.row_groups - 1) + (p.partials - 1);
    p.ws_bytes = (int64_t)p.partials * UC_DW_WS_ROWS * C * 4;
    return p;
}

// work item -> (vector of the chunk, tap row, row group); group >= row_groups: the item idles (the workgroup is rounded up to a wavefront)
struct DwconvWgradItem { int c8, ky, group; };
UC_DW_HD static inline DwconvWgradItem uc_dwconv_wgrad_item(int c8n, int tid) {
    DwconvWgradItem t;
    t.c8 = tid % c8n; tid /= c8n;
    t.ky = tid % 7;
    t.group = tid / 7;
    return t;
}
