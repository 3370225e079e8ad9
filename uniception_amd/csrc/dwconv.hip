// The depthwise 7x7 convolution of the ConvNeXt layer on channels-last maps (gfx950), its weight gradient, and the operand rows of the
// stage downsample Conv2d(k = 2, stride = 2).  A depthwise convolution reduces over no channel, so it is a streaming stencil on the
// vector ALU, not a matrix product: tile + halo staged once in LDS, 49 fp32 FMAs per output element, every output written once by a
// plain 16-byte store.  No atomics, nothing allocated; every sum runs in one fixed order.  The geometry is csrc/dwconv_plan.h.
#include "vec_access.h"
#include "dwconv_plan.h"

// eight consecutive storage elements, moved as they lie in memory
template <typename Tag>
__device__ __forceinline__ void raw_copy8(typename Tag::storage* dst, const typename Tag::storage* src) {
    constexpr int N = (int)sizeof(typename Tag::storage) * 8 / 16;
#pragma unroll
    for (int n = 0; n < N; ++n) reinterpret_cast<uint4*>(dst)[n] = reinterpret_cast<const uint4*>(src)[n];
}
template <typename Tag>
__device__ __forceinline__ void raw_zero8(typename Tag::storage* dst) {
    constexpr int N = (int)sizeof(typename Tag::storage) * 8 / 16;
#pragma unroll
    for (int n = 0; n < N; ++n) reinterpret_cast<uint4*>(dst)[n] = make_uint4(0u, 0u, 0u, 0u);
}
__device__ __forceinline__ Vec8 dw_zero8() {
    Vec8 z;
#pragma unroll
    for (int e = 0; e < 8; ++e) z.v[e] = 0.f;
    return z;
}

// s[(ly * lw + lx) * stride + c8] <- x[b, y0 + ly, x0 + lx, (c8_0 + c8) * 8 ..], zeros outside the map and beyond C
template <typename Tag>
__device__ __forceinline__ void dw_stage(typename Tag::storage* s, const typename Tag::storage* __restrict__ x, int64_t b, int y0, int x0, int lh, int lw,
                                         int c8n, int stride, int c8_0, int H, int W, int C) {
    const int C8 = C / 8;
    for (int i = threadIdx.x; i < lh * lw * c8n; i += blockDim.x) {
        const int c8 = i % c8n, pix = i / c8n;
        const int gy = y0 + pix / lw, gx = x0 + pix % lw, gc8 = c8_0 + c8;
        typename Tag::storage* dst = s + ((int64_t)pix * stride + c8) * 8;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W && gc8 < C8) raw_copy8<Tag>(dst, x + ((b * H + gy) * W + gx) * (int64_t)C + gc8 * 8);
        else raw_zero8<Tag>(dst);
    }
}

// ---- forward (and, with flip, the data gradient) -------------------------------------------------------------------------------
template <typename Tag>
__global__ __launch_bounds__(UC_DW_MAX_THREADS) void dwconv7x7_kernel(const typename Tag::storage* __restrict__ x, const float* __restrict__ w,
                                                                     const float* __restrict__ bias, typename Tag::storage* __restrict__ y,
                                                                     int H, int W, int C, int flip, DwconvPlan pl) {
    extern __shared__ uint4 dw_lds[];
    typename Tag::storage* s_in = reinterpret_cast<typename Tag::storage*>(dw_lds);
    float* s_w = reinterpret_cast<float*>(reinterpret_cast<char*>(dw_lds) + pl.lds_in_bytes);
    const DwconvBlock k = uc_dwconv_block(pl.tiles_x, pl.tiles_y, pl.chunks, blockIdx.x);
    const int C8 = C / 8, c8_0 = k.chunk * pl.c8;
    const int lw = pl.tile_w + 2 * UC_DW_RADIUS, lh = pl.tile_h + 2 * UC_DW_RADIUS;
    dw_stage<Tag>(s_in, x, k.b, k.ty * pl.tile_h - UC_DW_RADIUS, k.tx * pl.tile_w - UC_DW_RADIUS, lh, lw, pl.c8, pl.pix_stride, c8_0, H, W, C);
    for (int i = threadIdx.x; i < UC_DW_TAPS * pl.c8; i += blockDim.x) {
        const int c8 = i % pl.c8, t = i / pl.c8, gc8 = c8_0 + c8;
        float* dst = s_w + (int64_t)i * 8;
        if (gc8 < C8) raw_copy8<F32Tag>(dst, w + (int64_t)(flip ? UC_DW_TAPS - 1 - t : t) * C + gc8 * 8);
        else raw_zero8<F32Tag>(dst);
    }
    __syncthreads();
    for (int it = threadIdx.x; it < pl.items; it += blockDim.x) {
        const DwconvItem m = uc_dwconv_item(pl.c8, pl.tile_w, it);
        const int gc8 = c8_0 + m.c8, gy = k.ty * pl.tile_h + m.row, gx0 = k.tx * pl.tile_w + m.run * UC_DW_RUN;
        if (gc8 >= C8 || gy >= H || gx0 >= W) continue;
        Vec8 acc[UC_DW_RUN];
        acc[0] = bias ? vec_load8<F32Tag>(bias + gc8 * 8) : dw_zero8();
#pragma unroll
        for (int r = 1; r < UC_DW_RUN; ++r) acc[r] = acc[0];
#pragma unroll 1
        for (int ky = 0; ky < 7; ++ky) {
            Vec8 wv[7];
#pragma unroll
            for (int kx = 0; kx < 7; ++kx) wv[kx] = vec_load8<F32Tag>(s_w + ((ky * 7 + kx) * pl.c8 + m.c8) * 8);
            const typename Tag::storage* rowp = s_in + (((int64_t)(m.row + ky) * lw + m.run * UC_DW_RUN) * pl.pix_stride + m.c8) * 8;
#pragma unroll
            for (int q = 0; q < UC_DW_RUN + 6; ++q) {            // input column q of the run feeds output r through tap kx = q - r
                const Vec8 v = vec_load8<Tag>(rowp + (int64_t)q * pl.pix_stride * 8);
#pragma unroll
                for (int r = 0; r < UC_DW_RUN; ++r) {
                    const int kx = q - r;
                    if (kx >= 0 && kx < 7) {
#pragma unroll
                        for (int e = 0; e < 8; ++e) acc[r].v[e] = fmaf(wv[kx].v[e], v.v[e], acc[r].v[e]);
                    }
                }
            }
        }
        typename Tag::storage* out = y + ((k.b * (int64_t)H + gy) * W + gx0) * (int64_t)C + gc8 * 8;
#pragma unroll
        for (int r = 0; r < UC_DW_RUN; ++r)
            if (gx0 + r < W) vec_store8<Tag>(out + (int64_t)r * C, acc[r]);
    }
}

// ---- weight gradient -------------------------------------------------------------------------------------------------------------
template <typename Tag>
__global__ __launch_bounds__(UC_DW_MAX_THREADS) void dwconv7x7_wgrad_kernel(const typename Tag::storage* __restrict__ x, const typename Tag::storage* __restrict__ dy,
                                                                           float* __restrict__ ws, int H, int W, int C, DwconvWgradPlan pl) {
    extern __shared__ uint4 dw_lds[];
    typename Tag::storage* s_x = reinterpret_cast<typename Tag::storage*>(dw_lds);
    typename Tag::storage* s_dy = reinterpret_cast<typename Tag::storage*>(reinterpret_cast<char*>(dw_lds) + pl.lds_x_bytes);
    float* s_red = reinterpret_cast<float*>(reinterpret_cast<char*>(dw_lds) + pl.lds_x_bytes + pl.lds_dy_bytes);
    const int part = blockIdx.x, chunk = blockIdx.y;
    const int C8 = C / 8, c8_0 = chunk * pl.c8;
    const int lw = pl.tile_w + 2 * UC_DW_RADIUS, lh = pl.tile_h + 2 * UC_DW_RADIUS;
    const DwconvWgradItem m = uc_dwconv_wgrad_item(pl.c8, threadIdx.x);
    const bool active = m.group < pl.row_groups && c8_0 + m.c8 < C8;
    Vec8 acc[7], accb = dw_zero8();
#pragma unroll
    for (int kx = 0; kx < 7; ++kx) acc[kx] = dw_zero8();
    for (int64_t u = part; u < pl.units; u += pl.partials) {
        const int tx = (int)(u % pl.tiles_x), ty = (int)((u / pl.tiles_x) % pl.tiles_y);
        const int64_t b = u / ((int64_t)pl.tiles_x * pl.tiles_y);
        __syncthreads();            // (the previous unit's readers are done)
        dw_stage<Tag>(s_x, x, b, ty * pl.tile_h - UC_DW_RADIUS, tx * pl.tile_w - UC_DW_RADIUS, lh, lw, pl.c8, pl.pix_stride, c8_0, H, W, C);
        dw_stage<Tag>(s_dy, dy, b, ty * pl.tile_h, tx * pl.tile_w, pl.tile_h, pl.tile_w, pl.c8, pl.pix_stride, c8_0, H, W, C);
        __syncthreads();
        if (!active) continue;
        for (int row = m.group; row < pl.tile_h; row += pl.row_groups) {
            for (int j0 = 0; j0 < pl.tile_w; j0 += UC_DW_RUN) {
                Vec8 d[UC_DW_RUN];
#pragma unroll
                for (int r = 0; r < UC_DW_RUN; ++r) d[r] = vec_load8<Tag>(s_dy + (((int64_t)row * pl.tile_w + j0 + r) * pl.pix_stride + m.c8) * 8);
                if (m.ky == 0) {
#pragma unroll
                    for (int r = 0; r < UC_DW_RUN; ++r)
#pragma unroll
                        for (int e = 0; e < 8; ++e) accb.v[e] += d[r].v[e];
                }
                const typename Tag::storage* rowp = s_x + (((int64_t)(row + m.ky) * lw + j0) * pl.pix_stride + m.c8) * 8;
#pragma unroll
                for (int q = 0; q < UC_DW_RUN + 6; ++q) {
                    const Vec8 v = vec_load8<Tag>(rowp + (int64_t)q * pl.pix_stride * 8);
#pragma unroll
                    for (int r = 0; r < UC_DW_RUN; ++r) {
                        const int kx = q - r;
                        if (kx >= 0 && kx < 7) {
#pragma unroll
                            for (int e = 0; e < 8; ++e) acc[kx].v[e] = fmaf(d[r].v[e], v.v[e], acc[kx].v[e]);
                        }
                    }
                }
            }
        }
    }
    // row groups 1, 2, ... are added to group 0 in that order through s_red [50][c8][8]
    for (int g = 1; g < pl.row_groups; ++g) {
        __syncthreads();
        if (active && m.group == g) {
#pragma unroll
            for (int kx = 0; kx < 7; ++kx) vec_store8<F32Tag>(s_red + ((m.ky * 7 + kx) * pl.c8 + m.c8) * 8, acc[kx]);
            if (m.ky == 0) vec_store8<F32Tag>(s_red + (UC_DW_TAPS * pl.c8 + m.c8) * 8, accb);
        }
        __syncthreads();
        if (active && m.group == 0) {
#pragma unroll
            for (int kx = 0; kx < 7; ++kx) {
                const Vec8 o = vec_load8<F32Tag>(s_red + ((m.ky * 7 + kx) * pl.c8 + m.c8) * 8);
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[kx].v[e] += o.v[e];
            }
            if (m.ky == 0) {
                const Vec8 o = vec_load8<F32Tag>(s_red + (UC_DW_TAPS * pl.c8 + m.c8) * 8);
#pragma unroll
                for (int e = 0; e < 8; ++e) accb.v[e] += o.v[e];
            }
        }
    }
    if (active && m.group == 0) {
        float* out = ws + (int64_t)part * UC_DW_WS_ROWS * C + (c8_0 + m.c8) * 8;
#pragma unroll
        for (int kx = 0; kx < 7; ++kx) vec_store8<F32Tag>(out + (int64_t)(m.ky * 7 + kx) * C, acc[kx]);
        if (m.ky == 0) vec_store8<F32Tag>(out + (int64_t)UC_DW_TAPS * C, accb);
    }
}

// dw [49][C], db [C] <- ws [partials][50][C], partials ascending
__global__ __launch_bounds__(256) void dwconv7x7_wgrad_merge_kernel(const float* __restrict__ ws, float* __restrict__ dw, float* __restrict__ db, int C, int partials) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= UC_DW_WS_ROWS * C) return;
    float s = 0.f;
    for (int q = 0; q < partials; ++q) s += ws[(int64_t)q * UC_DW_WS_ROWS * C + i];
    if (i < UC_DW_TAPS * C) dw[i] = s;
    else if (db) db[i - UC_DW_TAPS * C] = s;
}

// ---- operand rows of Conv2d(k = 2, stride = 2) -----------------------------------------------------------------------------------
// rows [B Ho Wo, 4 C]: work item = 8 channels of one tap of one output pixel (index space [B Ho Wo, 4, C8]: the store is contiguous)
template <typename Tag>
__global__ __launch_bounds__(256) void patch2_gather_kernel(const typename Tag::storage* __restrict__ x, typename Tag::storage* __restrict__ rows,
                                                            int H, int W, int C, int64_t items) {
    const int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (it >= items) return;
    const int C8 = C / 8, Ho = H / 2, Wo = W / 2;
    int64_t r = it;
    const int c8 = (int)(r % C8); r /= C8;
    const int tap = (int)(r % 4); r /= 4;
    const int j = (int)(r % Wo); r /= Wo;
    const int i = (int)(r % Ho);
    const int64_t b = r / Ho;
    raw_copy8<Tag>(rows + it * 8, x + ((b * H + 2 * i + tap / 2) * W + 2 * j + tap % 2) * (int64_t)C + c8 * 8);
}

// dx [B, H, W, C]: pixel (y, x) is read by exactly one row entry, or (odd last row / column) by none
template <typename Tag>
__global__ __launch_bounds__(256) void patch2_gather_bwd_kernel(const typename Tag::storage* __restrict__ drows, typename Tag::storage* __restrict__ dx,
                                                                int H, int W, int C, int64_t items) {
    const int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (it >= items) return;
    const int C8 = C / 8, Ho = H / 2, Wo = W / 2;
    int64_t r = it;
    const int c8 = (int)(r % C8); r /= C8;
    const int xx = (int)(r % W); r /= W;
    const int yy = (int)(r % H);
    const int64_t b = r / H;
    if (yy < 2 * Ho && xx < 2 * Wo)
        raw_copy8<Tag>(dx + it * 8, drows + ((((b * Ho + yy / 2) * Wo + xx / 2) * 4 + (yy & 1) * 2 + (xx & 1)) * (int64_t)C + c8 * 8));
    else
        raw_zero8<Tag>(dx + it * 8);
}

// ---- entry points ----------------------------------------------------------------------------------------------------------------
static int dw_check(const char* fn, int dtype, int B, int H, int W, int C) {
    UC_REQUIRE_DTYPE(fn, dtype, true);
    UC_REQUIRE(B >= 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0, "%s: bad shape B=%d H=%d W=%d C=%d (C must be a multiple of 8)", fn, B, H, W, C);
    UC_REQUIRE(H <= 0x3ffffff0 && W <= 0x3ffffff0 && (int64_t)B * H * W * (C / 8) <= 0x7fffffff, "%s: grid limit exceeded (B H W C / 8 must stay below 2^31)", fn);
    return UC_OK;
}
#define DW_ALIGNED(p) ((uintptr_t)(p) % 16 == 0)

extern "C" int uc_dwconv7x7_nhwc(const void* x, const float* w, const float* bias, void* y, int dtype, int B, int H, int W, int C, int flip,
                                 uc_stream_t stream) {
    const char* fn = "uc_dwconv7x7_nhwc";
    if (int e = dw_check(fn, dtype, B, H, W, C)) return e;
    if (B == 0) return UC_OK;
    UC_REQUIRE(x && w && y, "%s: null pointer", fn);
    UC_REQUIRE(DW_ALIGNED(x) && DW_ALIGNED(w) && DW_ALIGNED(y) && DW_ALIGNED(bias), "%s: x, w, bias and y must be 16-byte aligned", fn);
    UC_REQUIRE(x != y, "%s: y == x (the convolution does not run in place)", fn);
    const DwconvPlan pl = uc_dwconv_plan(dtype, B, H, W, C);
    UC_REQUIRE(pl.grid <= 0x7fffffff && pl.lds_bytes <= UC_DW_LDS_BUDGET, "%s: grid limit exceeded", fn);
    UC_DISPATCH_F16(fn, dtype, hipLaunchKernelGGL(dwconv7x7_kernel<Tag>, dim3((unsigned)pl.grid), dim3(pl.threads), pl.lds_bytes, (hipStream_t)stream,
                                                   (const Tag::storage*)x, w, bias, (Tag::storage*)y, H, W, C, flip != 0, pl));
    UC_CHECK_LAUNCH(fn);
    return UC_OK;
}

extern "C" int64_t uc_dwconv7x7_nhwc_wgrad_ws_bytes(int64_t B, int64_t H, int64_t W, int64_t C) {
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8 != 0 || H > 0x3ffffff0 || W > 0x3ffffff0 || C > 0x3ffffff0) return 0;
    return uc_dwconv_wgrad_plan(UC_F32, B, (int)H, (int)W, (int)C).ws_bytes;      // (the partial count does not depend on the dtype)
}

extern "C" int uc_dwconv7x7_nhwc_wgrad(const void* x, const void* dy, float* dw, float* db, float* ws, int dtype, int B, int H, int W, int C,
                                       uc_stream_t stream) {
    const char* fn = "uc_dwconv7x7_nhwc_wgrad";
    if (int e = dw_check(fn, dtype, B, H, W, C)) return e;
    UC_REQUIRE(dw, "%s: null pointer", fn);
    UC_REQUIRE(DW_ALIGNED(dw) && DW_ALIGNED(db), "%s: dw and db must be 16-byte aligned", fn);
    UC_REQUIRE(UC_DW_WS_ROWS * (int64_t)C <= 0x7fffffff - 256, "%s: grid limit exceeded", fn);
    hipStream_t st = (hipStream_t)stream;
    const unsigned mgrid = (unsigned)((UC_DW_WS_ROWS * (int64_t)C + 255) / 256);
    if (B == 0) return UC_OK;
    UC_REQUIRE(x && dy && ws, "%s: null pointer", fn);
    UC_REQUIRE(DW_ALIGNED(x) && DW_ALIGNED(dy) && DW_ALIGNED(ws), "%s: x, dy and ws must be 16-byte aligned", fn);
    const DwconvWgradPlan pl = uc_dwconv_wgrad_plan(dtype, B, H, W, C);
    UC_REQUIRE(pl.lds_bytes <= UC_DW_LDS_BUDGET && pl.chunks <= 65535, "%s: grid limit exceeded", fn);
    UC_DISPATCH_F16(fn, dtype, hipLaunchKernelGGL(dwconv7x7_wgrad_kernel<Tag>, dim3((unsigned)pl.partials, (unsigned)pl.chunks), dim3(pl.threads), pl.lds_bytes, st,
                                                   (const Tag::storage*)x, (const Tag::storage*)dy, ws, H, W, C, pl));
    UC_CHECK_LAUNCH(fn);
    hipLaunchKernelGGL(dwconv7x7_wgrad_merge_kernel, dim3(mgrid), dim3(256), 0, st, (const float*)ws, dw, db, C, pl.partials);
    UC_CHECK_LAUNCH(fn);
    return UC_OK;
}

static int p2_check(const char* fn, const void* a, const void* b, int dtype, int B, int H, int W, int C) {
    if (int e = dw_check(fn, dtype, B, H, W, C)) return e;
    UC_REQUIRE(DW_ALIGNED(a) && DW_ALIGNED(b), "%s: maps must be 16-byte aligned", fn);
    return UC_OK;
}
#define DW_GRID(items) dim3((unsigned)(((items) + 255) / 256))

extern "C" int uc_patch2_gather_nhwc(const void* x, void* rows, int dtype, int B, int H, int W, int C, uc_stream_t stream) {
    const char* fn = "uc_patch2_gather_nhwc";
    if (int e = p2_check(fn, x, rows, dtype, B, H, W, C)) return e;
    const int64_t items = (int64_t)B * (H / 2) * (W / 2) * 4 * (C / 8);
    if (items == 0) return UC_OK;           // (no image, or a map of one row / column: no rows)
    UC_REQUIRE(x && rows, "%s: null pointer", fn);
    UC_DISPATCH_F16(fn, dtype, hipLaunchKernelGGL(patch2_gather_kernel<Tag>, DW_GRID(items), dim3(256), 0, (hipStream_t)stream, (const Tag::storage*)x, (Tag::storage*)rows, H, W, C, items));
    UC_CHECK_LAUNCH(fn);
    return UC_OK;
}

extern "C" int uc_patch2_gather_nhwc_bwd(const void* drows, void* dx, int dtype, int B, int H, int W, int C, uc_stream_t stream) {
    const char* fn = "uc_patch2_gather_nhwc_bwd";
    if (int e = p2_check(fn, dx, dx, dtype, B, H, W, C)) return e;
    const int64_t items = (int64_t)B * H * W * (C / 8);
    if (items == 0) return UC_OK;
    UC_REQUIRE(dx && (drows || (H / 2) * (int64_t)(W / 2) == 0), "%s: null pointer", fn);
    UC_REQUIRE(DW_ALIGNED(drows), "%s: drows must be 16-byte aligned", fn);
    UC_DISPATCH_F16(fn, dtype, hipLaunchKernelGGL(patch2_gather_bwd_kernel<Tag>, DW_GRID(items), dim3(256), 0, (hipStream_t)stream, (const Tag::storage*)drows, (Tag::storage*)dx, H, W, C, items));
    UC_CHECK_LAUNCH(fn);
    return UC_OK;
}
