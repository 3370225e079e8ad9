// Channels-last data movement of the MoGe head (gfx950): replicate padding by one pixel and its adjoint, the crop (+ residual) that
// undoes it and its adjoint, and the bilinear resize with PyTorch's half-pixel rule (align_corners=False) and its adjoint.
// One work item = 8 consecutive channels of one DESTINATION pixel (vec_access.h): 16-byte accesses, consecutive lanes on consecutive
// addresses, every output element written once by a plain vector store; the adjoints are gathers in a fixed order (no atomics).
//
// A replicate-padded 3x3 convolution is  pad -> the zero-padded 3x3 convolution of uc_gemm on the (H + 2) x (W + 2) map -> crop:
// every tap of an interior output reads a real element of the padded map, so the interior IS the replicate-padded convolution.
#include "vec_access.h"

// item -> (b, y, x, c8) of a [B, Hd, Wd, C8] index space
struct PixIdx { int64_t b; int y, x, c8; };
__device__ __forceinline__ PixIdx pix_of(int64_t it, int Hd, int Wd, int C8) {
    PixIdx p;
    int64_t r = it;
    p.c8 = (int)(r % C8); r /= C8;
    p.x = (int)(r % Wd); r /= Wd;
    p.y = (int)(r % Hd);
    p.b = r / Hd;
    return p;
}

// dst [B, H + 2, W + 2, C] <- src [B, H, W, C], dst[b, y, x] = src[b, clamp(y - 1), clamp(x - 1)]
template <typename Tag>
__global__ __launch_bounds__(256) void replicate_pad_kernel(const typename Tag::storage* __restrict__ src, typename Tag::storage* __restrict__ dst,
                                                            int H, int W, int C, int64_t items) {
    const int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (it >= items) return;
    const PixIdx p = pix_of(it, H + 2, W + 2, C / 8);
    const int sy = min(max(p.y - 1, 0), H - 1), sx = min(max(p.x - 1, 0), W - 1);
    vec_store8<Tag>(dst + it * 8, vec_load8<Tag>(src + ((p.b * H + sy) * W + sx) * (int64_t)C + p.c8 * 8));
}

// dx [B, H, W, C] <- dy [B, H + 2, W + 2, C]: an interior pixel sums the padded positions that clamp to it (rows ascending, then
// columns ascending: 1, 2 on an edge, 4 at a corner; more when H or W is 1)
template <typename Tag>
__global__ __launch_bounds__(256) void replicate_pad_bwd_kernel(const typename Tag::storage* __restrict__ dy, typename Tag::storage* __restrict__ dx,
                                                                int H, int W, int C, int64_t items) {
    const int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (it >= items) return;
    const PixIdx p = pix_of(it, H, W, C / 8);
    const int y0 = p.y == 0 ? 0 : p.y + 1, y1 = p.y == H - 1 ? H + 1 : p.y + 1;
    const int x0 = p.x == 0 ? 0 : p.x + 1, x1 = p.x == W - 1 ? W + 1 : p.x + 1;
    Vec8 acc;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc.v[e] = 0.f;
    const typename Tag::storage* base = dy + p.b * (H + 2) * (int64_t)(W + 2) * C + p.c8 * 8;
    for (int yy = y0; yy <= y1; ++yy)
        for (int xx = x0; xx <= x1; ++xx) {
            const Vec8 g = vec_load8<Tag>(base + ((int64_t)yy * (W + 2) + xx) * C);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc.v[e] += g.v[e];
        }
    vec_store8<Tag>(dx + it * 8, acc);
}

// dst [B, H, W, C] = act(src[B, H + 2, W + 2, C] interior (+ residual [B, H, W, C]))
template <typename Tag, bool RES, bool RELU>
__global__ __launch_bounds__(256) void crop_add_kernel(const typename Tag::storage* __restrict__ src, const typename Tag::storage* __restrict__ res,
                                                       typename Tag::storage* __restrict__ dst, int H, int W, int C, int64_t items) {
    const int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (it >= items) return;
    const PixIdx p = pix_of(it, H, W, C / 8);
    Vec8 v = vec_load8<Tag>(src + ((p.b * (H + 2) + p.y + 1) * (W + 2) + p.x + 1) * (int64_t)C + p.c8 * 8);
    if (RES) {
        const Vec8 r = vec_load8<Tag>(res + it * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) v.v[e] += r.v[e];
    }
    if (RELU) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v.v[e] = fmaxf(v.v[e], 0.f);
    }
    vec_store8<Tag>(dst + it * 8, v);
}

// dst [B, H + 2, W + 2, C]: dy [B, H, W, C] in the interior, zeros on the ring
template <typename Tag>
__global__ __launch_bounds__(256) void crop_embed_kernel(const typename Tag::storage* __restrict__ dy, typename Tag::storage* __restrict__ dst,
                                                         int H, int W, int C, int64_t items) {
    const int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (it >= items) return;
    const PixIdx p = pix_of(it, H + 2, W + 2, C / 8);
    Vec8 v;
    if (p.y >= 1 && p.y <= H && p.x >= 1 && p.x <= W) {
        v = vec_load8<Tag>(dy + ((p.b * H + p.y - 1) * W + p.x - 1) * (int64_t)C + p.c8 * 8);
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) v.v[e] = 0.f;
    }
    vec_store8<Tag>(dst + it * 8, v);
}

// ---- half-pixel bilinear resize ------------------------------------------------------------------------------------------------------
// src coordinate of destination index d: max(0, (d + 0.5) in / out - 0.5) = max(0, ((2 d + 1) in - out) / (2 out)), evaluated in
// integers: i0 = the quotient, lambda = remainder / (2 out) (one rounding), i1 = min(i0 + 1, in - 1).
__device__ __forceinline__ void halfpix_tap(int d, int in, int out, int& i0, int& i1, float& lam) {
    const int num = (2 * d + 1) * in - out;
    if (num <= 0) { i0 = 0; lam = 0.f; }
    else {
        i0 = num / (2 * out);
        lam = (float)(num - i0 * 2 * out) / (float)(2 * out);
    }
    i1 = min(i0 + 1, in - 1);
}

template <typename Tag>
__global__ __launch_bounds__(256) void resize_halfpix_kernel(const typename Tag::storage* __restrict__ src, typename Tag::storage* __restrict__ dst,
                                                             int Hi, int Wi, int C, int Ho, int Wo, int64_t items) {
    const int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (it >= items) return;
    const PixIdx p = pix_of(it, Ho, Wo, C / 8);
    int y0, y1, x0, x1;
    float ly, lx;
    halfpix_tap(p.y, Hi, Ho, y0, y1, ly);
    halfpix_tap(p.x, Wi, Wo, x0, x1, lx);
    const float hy = 1.f - ly, hx = 1.f - lx;
    const typename Tag::storage* base = src + p.b * Hi * (int64_t)Wi * C + p.c8 * 8;
    const Vec8 p00 = vec_load8<Tag>(base + ((int64_t)y0 * Wi + x0) * C), p01 = vec_load8<Tag>(base + ((int64_t)y0 * Wi + x1) * C);
    const Vec8 p10 = vec_load8<Tag>(base + ((int64_t)y1 * Wi + x0) * C), p11 = vec_load8<Tag>(base + ((int64_t)y1 * Wi + x1) * C);
    Vec8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o.v[e] = hy * (hx * p00.v[e] + lx * p01.v[e]) + ly * (hx * p10.v[e] + lx * p11.v[e]);
    vec_store8<Tag>(dst + it * 8, o);
}

// destination indices whose taps can touch source index i: a superset, the exact weights are re-evaluated per candidate
__device__ __forceinline__ void halfpix_range(int i, int in, int out, int& lo, int& hi) {
    lo = max(0, (int)(((int64_t)(i - 1) * out) / in) - 2);
    hi = min(out - 1, (int)(((int64_t)(i + 2) * out) / in) + 2);
}

// gather form of the adjoint: one work item = 8 channels of one SOURCE pixel, output rows ascending, then columns ascending
template <typename Tag>
__global__ __launch_bounds__(256) void resize_halfpix_bwd_kernel(const typename Tag::storage* __restrict__ dy, typename Tag::storage* __restrict__ dx,
                                                                 int Hi, int Wi, int C, int Ho, int Wo, int64_t items) {
    const int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (it >= items) return;
    const PixIdx p = pix_of(it, Hi, Wi, C / 8);
    int ylo, yhi, xlo, xhi;
    halfpix_range(p.y, Hi, Ho, ylo, yhi);
    halfpix_range(p.x, Wi, Wo, xlo, xhi);
    Vec8 acc;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc.v[e] = 0.f;
    const typename Tag::storage* base = dy + p.b * Ho * (int64_t)Wo * C + p.c8 * 8;
    for (int oy = ylo; oy <= yhi; ++oy) {
        int y0, y1;
        float ly;
        halfpix_tap(oy, Hi, Ho, y0, y1, ly);
        const float wy = (y0 == p.y ? 1.f - ly : 0.f) + (y1 == p.y ? ly : 0.f);
        if (wy == 0.f) continue;
        for (int ox = xlo; ox <= xhi; ++ox) {
            int x0, x1;
            float lx;
            halfpix_tap(ox, Wi, Wo, x0, x1, lx);
            const float wx = (x0 == p.x ? 1.f - lx : 0.f) + (x1 == p.x ? lx : 0.f);
            if (wx == 0.f) continue;
            const Vec8 g = vec_load8<Tag>(base + ((int64_t)oy * Wo + ox) * C);
            const float w = wy * wx;
#pragma unroll
            for (int e = 0; e < 8; ++e) acc.v[e] = fmaf(w, g.v[e], acc.v[e]);
        }
    }
    vec_store8<Tag>(dx + it * 8, acc);
}

// ---- entry points ----------------------------------------------------------------------------------------------------------------
static int pr_check(const char* fn, const void* a, const void* b, int dtype, int B, int H, int W, int C, int64_t items) {
    UC_REQUIRE(a && b, "%s: null pointer", fn);
    UC_REQUIRE_DTYPE(fn, dtype, true);
    UC_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0, "%s: bad shape B=%d H=%d W=%d C=%d (C must be a multiple of 8)", fn, B, H, W, C);
    UC_REQUIRE((uintptr_t)a % 16 == 0 && (uintptr_t)b % 16 == 0, "%s: maps must be 16-byte aligned", fn);
    UC_REQUIRE(H <= 0x3ffffff0 && W <= 0x3ffffff0 && (items + 255) / 256 <= 0x7fffffff, "%s: grid limit exceeded", fn);
    return UC_OK;
}
#define PR_GRID(items) dim3((unsigned)(((items) + 255) / 256))

extern "C" int uc_replicate_pad_nhwc(const void* src, void* dst, int dtype, int B, int H, int W, int C, uc_stream_t stream) {
    const char* fn = "uc_replicate_pad_nhwc";
    const int64_t items = (int64_t)B * ((int64_t)H + 2) * ((int64_t)W + 2) * (C / 8);
    if (int e = pr_check(fn, src, dst, dtype, B, H, W, C, items)) return e;
    UC_DISPATCH_F16(fn, dtype, hipLaunchKernelGGL(replicate_pad_kernel<Tag>, PR_GRID(items), dim3(256), 0, (hipStream_t)stream, (const Tag::storage*)src, (Tag::storage*)dst, H, W, C, items));
    UC_CHECK_LAUNCH(fn);
    return UC_OK;
}

extern "C" int uc_replicate_pad_nhwc_bwd(const void* dy, void* dx, int dtype, int B, int H, int W, int C, uc_stream_t stream) {
    const char* fn = "uc_replicate_pad_nhwc_bwd";
    const int64_t items = (int64_t)B * H * W * (C / 8);
    if (int e = pr_check(fn, dy, dx, dtype, B, H, W, C, (int64_t)B * ((int64_t)H + 2) * ((int64_t)W + 2) * (C / 8))) return e;
    UC_DISPATCH_F16(fn, dtype, hipLaunchKernelGGL(replicate_pad_bwd_kernel<Tag>, PR_GRID(items), dim3(256), 0, (hipStream_t)stream, (const Tag::storage*)dy, (Tag::storage*)dx, H, W, C, items));
    UC_CHECK_LAUNCH(fn);
    return UC_OK;
}

extern "C" int uc_crop_add_nhwc(const void* src, const void* residual, void* dst, int dtype, int B, int H, int W, int C, int relu,
                                uc_stream_t stream) {
    const char* fn = "uc_crop_add_nhwc";
    const int64_t items = (int64_t)B * H * W * (C / 8);
    if (int e = pr_check(fn, src, dst, dtype, B, H, W, C, (int64_t)B * ((int64_t)H + 2) * ((int64_t)W + 2) * (C / 8))) return e;
    UC_REQUIRE(!residual || (uintptr_t)residual % 16 == 0, "%s: residual must be 16-byte aligned", fn);
    hipStream_t st = (hipStream_t)stream;
    if (residual && relu)
        UC_DISPATCH_F16(fn, dtype, hipLaunchKernelGGL((crop_add_kernel<Tag, true, true>), PR_GRID(items), dim3(256), 0, st, (const Tag::storage*)src, (const Tag::storage*)residual, (Tag::storage*)dst, H, W, C, items));
    else if (residual)
        UC_DISPATCH_F16(fn, dtype, hipLaunchKernelGGL((crop_add_kernel<Tag, true, false>), PR_GRID(items), dim3(256), 0, st, (const Tag::storage*)src, (const Tag::storage*)residual, (Tag::storage*)dst, H, W, C, items));
    else if (relu)
        UC_DISPATCH_F16(fn, dtype, hipLaunchKernelGGL((crop_add_kernel<Tag, false, true>), PR_GRID(items), dim3(256), 0, st, (const Tag::storage*)src, (const Tag::storage*)nullptr, (Tag::storage*)dst, H, W, C, items));
    else
        UC_DISPATCH_F16(fn, dtype, hipLaunchKernelGGL((crop_add_kernel<Tag, false, false>), PR_GRID(items), dim3(256), 0, st, (const Tag::storage*)src, (const Tag::storage*)nullptr, (Tag::storage*)dst, H, W, C, items));
    UC_CHECK_LAUNCH(fn);
    return UC_OK;
}

extern "C" int uc_crop_embed_nhwc(const void* dy, void* dst, int dtype, int B, int H, int W, int C, uc_stream_t stream) {
    const char* fn = "uc_crop_embed_nhwc";
    const int64_t items = (int64_t)B * ((int64_t)H + 2) * ((int64_t)W + 2) * (C / 8);
    if (int e = pr_check(fn, dy, dst, dtype, B, H, W, C, items)) return e;
    UC_DISPATCH_F16(fn, dtype, hipLaunchKernelGGL(crop_embed_kernel<Tag>, PR_GRID(items), dim3(256), 0, (hipStream_t)stream, (const Tag::storage*)dy, (Tag::storage*)dst, H, W, C, items));
    UC_CHECK_LAUNCH(fn);
    return UC_OK;
}

extern "C" int uc_resize_bilinear_nhwc(const void* src, void* dst, int dtype, int B, int Hi, int Wi, int C, int Ho, int Wo, int align_corners,
                                       uc_stream_t stream) {
    const char* fn = "uc_resize_bilinear_nhwc";
    if (align_corners) return uc_bilinear_nhwc(src, dst, dtype, B, Hi, Wi, C, Ho, Wo, Ho, Wo, stream);     // the DPT kernels, bit for bit
    const int64_t items = (int64_t)B * Ho * Wo * (C / 8);
    if (int e = pr_check(fn, src, dst, dtype, B, Hi, Wi, C, items)) return e;
    UC_REQUIRE(Ho > 0 && Wo > 0 && Ho <= 0x3ffffff0 && Wo <= 0x3ffffff0 && (int64_t)(2 * (int64_t)Ho + 1) * Hi < 0x7fffffff &&
                   (int64_t)(2 * (int64_t)Wo + 1) * Wi < 0x7fffffff,
               "%s: bad output size Ho=%d Wo=%d (2 * out * in must stay below 2^31)", fn, Ho, Wo);
    UC_DISPATCH_F16(fn, dtype, hipLaunchKernelGGL(resize_halfpix_kernel<Tag>, PR_GRID(items), dim3(256), 0, (hipStream_t)stream, (const Tag::storage*)src, (Tag::storage*)dst, Hi, Wi, C, Ho, Wo, items));
    UC_CHECK_LAUNCH(fn);
    return UC_OK;
}

extern "C" int uc_resize_bilinear_nhwc_bwd(const void* dy, void* dx, int dtype, int B, int Hi, int Wi, int C, int Ho, int Wo, int align_corners,
                                           uc_stream_t stream) {
    const char* fn = "uc_resize_bilinear_nhwc_bwd";
    if (align_corners) return uc_bilinear_nhwc_bwd(dy, dx, dtype, B, Hi, Wi, C, Ho, Wo, Ho, Wo, stream);
    const int64_t items = (int64_t)B * Hi * Wi * (C / 8);
    if (int e = pr_check(fn, dy, dx, dtype, B, Hi, Wi, C, items)) return e;
    UC_REQUIRE(Ho > 0 && Wo > 0 && Ho <= 0x3ffffff0 && Wo <= 0x3ffffff0 && (int64_t)(2 * (int64_t)Ho + 1) * Hi < 0x7fffffff &&
                   (int64_t)(2 * (int64_t)Wo + 1) * Wi < 0x7fffffff && ((int64_t)B * Ho * Wo * (C / 8) + 255) / 256 <= 0x7fffffff,
               "%s: bad output size Ho=%d Wo=%d (2 * out * in must stay below 2^31)", fn, Ho, Wo);
    UC_DISPATCH_F16(fn, dtype, hipLaunchKernelGGL(resize_halfpix_bwd_kernel<Tag>, PR_GRID(items), dim3(256), 0, (hipStream_t)stream, (const Tag::storage*)dy, (Tag::storage*)dx, Hi, Wi, C, Ho, Wo, items));
    UC_CHECK_LAUNCH(fn);
    return UC_OK;
}
