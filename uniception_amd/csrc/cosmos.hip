// Streaming passes of the Cosmos continuous image tokenizer (gfx950): the two-level Haar patcher and its inverse, the operand gather of
// the stride-2 Downsample convolution and its adjoint, the nearest-neighbour x2 upsample and its adjoint, and the row softmax (+ backward)
// of the single-head attention over all pixels.  All of them are bandwidth-bound: one work item moves 16 bytes per access
// (vec_access.h), every output element is written once by a plain vector store, and the adjoints are gathers in a fixed order
// (no atomics: the same bits on every run).
#include "vec_access.h"

// ---- Haar patcher --------------------------------------------------------------------------------------------------------------------
// One level on a 2x2 block (first index the row):  ll, lh, hl, hh = (x00 +- x01 +- x10 +- x11) / 4 with the signs of the 4x4 Hadamard
// matrix H4 (rows: ++++, ++--, +-+-, +--+).  The patcher is H4 / 4 per level, its inverse H4 itself (H4 H4 = 4 I).
__device__ __forceinline__ void haar4(float a, float b, float c, float d, float& ll, float& lh, float& hl, float& hh) {
    const float s0 = a + b, s1 = c + d, d0 = a - b, d1 = c - d;
    ll = s0 + s1; lh = s0 - s1; hl = d0 + d1; hh = d0 - d1;
}

// work item = one 4x4 block of one channel; consecutive lanes take consecutive blocks of an image row (16-byte loads side by side).
// grid-stride free: items = B * C * (H/4) * (W/4).
template <typename Tag>
__global__ __launch_bounds__(256) void haar_patch_kernel(const float* __restrict__ img, typename Tag::storage* __restrict__ rows, int C, int H, int W,
                                                         int ld, float scale, int64_t items) {
    const int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (it >= items) return;
    const int w4 = W / 4, h4 = H / 4;
    int64_t r = it;
    const int j = (int)(r % w4); r /= w4;
    const int c = (int)(r % C); r /= C;
    const int i = (int)(r % h4);
    const int64_t b = r / h4;
    const float* src = img + ((b * C + c) * H + 4 * (int64_t)i) * W + 4 * j;
    float4_t x[4];
#pragma unroll
    for (int y = 0; y < 4; ++y) x[y] = *reinterpret_cast<const float4_t*>(src + (int64_t)y * W);
    // level 1 on the four 2x2 blocks (u, v) of the 4x4 block: l1[s1][u][v]
    float l1[4][2][2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        haar4(x[2 * u].x, x[2 * u].y, x[2 * u + 1].x, x[2 * u + 1].y, l1[0][u][0], l1[1][u][0], l1[2][u][0], l1[3][u][0]);
        haar4(x[2 * u].z, x[2 * u].w, x[2 * u + 1].z, x[2 * u + 1].w, l1[0][u][1], l1[1][u][1], l1[2][u][1], l1[3][u][1]);
    }
    typename Tag::storage* dst = rows + ((b * h4 + i) * (int64_t)w4 + j) * ld + c;
    const float f = scale * (1.f / 16.f);
#pragma unroll
    for (int s1 = 0; s1 < 4; ++s1) {
        float o[4];
        haar4(l1[s1][0][0], l1[s1][0][1], l1[s1][1][0], l1[s1][1][1], o[0], o[1], o[2], o[3]);
#pragma unroll
        for (int s2 = 0; s2 < 4; ++s2) Tag::store(dst + (s2 * 4 + s1) * C, o[s2] * f);
    }
    if (c == 0) {      // the zero columns [16 C, ld): 16 C and ld are multiples of 8
        Vec8 z;
#pragma unroll
        for (int e = 0; e < 8; ++e) z.v[e] = 0.f;
        for (int k = 16 * C; k < ld; k += 8) vec_store8<Tag>(dst + k, z);
    }
}

template <typename Tag>
__global__ __launch_bounds__(256) void haar_unpatch_kernel(const typename Tag::storage* __restrict__ rows, float* __restrict__ img, int C, int H, int W,
                                                           int ld, float scale, int64_t items) {
    const int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (it >= items) return;
    const int w4 = W / 4, h4 = H / 4;
    int64_t r = it;
    const int j = (int)(r % w4); r /= w4;
    const int c = (int)(r % C); r /= C;
    const int i = (int)(r % h4);
    const int64_t b = r / h4;
    const typename Tag::storage* src = rows + ((b * h4 + i) * (int64_t)w4 + j) * ld + c;
    // undo level 2: l1[s1][u][v] = H4 over s2
    float l1[4][2][2];
#pragma unroll
    for (int s1 = 0; s1 < 4; ++s1) {
        float p[4];
#pragma unroll
        for (int s2 = 0; s2 < 4; ++s2) p[s2] = Tag::load(src + (s2 * 4 + s1) * C) * scale;
        haar4(p[0], p[1], p[2], p[3], l1[s1][0][0], l1[s1][0][1], l1[s1][1][0], l1[s1][1][1]);
    }
    float x[4][4];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v)
            haar4(l1[0][u][v], l1[1][u][v], l1[2][u][v], l1[3][u][v], x[2 * u][2 * v], x[2 * u][2 * v + 1], x[2 * u + 1][2 * v], x[2 * u + 1][2 * v + 1]);
    float* dst = img + ((b * C + c) * H + 4 * (int64_t)i) * W + 4 * j;
#pragma unroll
    for (int y = 0; y < 4; ++y) *reinterpret_cast<float4_t*>(dst + (int64_t)y * W) = (float4_t){x[y][0], x[y][1], x[y][2], x[y][3]};
}

// ---- Downsample operand / nearest upsample ---------------------------------------------------------------------------------------------
// item -> (b, y, x, c8) of a [B, Hd, Wd, C8] index space
struct CsIdx { int64_t b; int y, x, c8; };
__device__ __forceinline__ CsIdx cs_idx(int64_t it, int Hd, int Wd, int C8) {
    CsIdx p;
    int64_t r = it;
    p.c8 = (int)(r % C8); r /= C8;
    p.x = (int)(r % Wd); r /= Wd;
    p.y = (int)(r % Hd);
    p.b = r / Hd;
    return p;
}
__device__ __forceinline__ Vec8 vec_zero8() {
    Vec8 z;
#pragma unroll
    for (int e = 0; e < 8; ++e) z.v[e] = 0.f;
    return z;
}

// rows [B Ho Wo, 9 C]: work item = 8 channels of one tap of one output pixel (index space [B Ho Wo, 9, C8]: the store is contiguous)
template <typename Tag>
__global__ __launch_bounds__(256) void down2_gather_kernel(const typename Tag::storage* __restrict__ x, typename Tag::storage* __restrict__ rows,
                                                           int H, int W, int C, int64_t items) {
    const int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (it >= items) return;
    const int C8 = C / 8, Ho = H / 2, Wo = W / 2;
    int64_t r = it;
    const int c8 = (int)(r % C8); r /= C8;
    const int tap = (int)(r % 9); r /= 9;
    const int j = (int)(r % Wo); r /= Wo;
    const int i = (int)(r % Ho);
    const int64_t b = r / Ho;
    const int y = 2 * i + tap / 3, xx = 2 * j + tap % 3;
    const Vec8 v = (y < H && xx < W) ? vec_load8<Tag>(x + ((b * H + y) * W + xx) * (int64_t)C + c8 * 8) : vec_zero8();
    vec_store8<Tag>(rows + it * 8, v);
}

// dx [B, H, W, C]: pixel (y, x) is read by output row i = (y - ky) / 2 for ky = y & 1 and, when y is even and >= 2, ky = 2
template <typename Tag>
__global__ __launch_bounds__(256) void down2_gather_bwd_kernel(const typename Tag::storage* __restrict__ drows, typename Tag::storage* __restrict__ dx,
                                                               int H, int W, int C, int64_t items) {
    const int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (it >= items) return;
    const int Ho = H / 2, Wo = W / 2;
    const CsIdx p = cs_idx(it, H, W, C / 8);
    Vec8 acc = vec_zero8();
    const int ky0 = p.y & 1, kx0 = p.x & 1;
    for (int ky = ky0; ky < 3; ky += 2) {
        const int i = (p.y - ky) / 2;
        if (p.y < ky) continue;
        for (int kx = kx0; kx < 3; kx += 2) {
            const int j = (p.x - kx) / 2;
            if (p.x < kx) continue;
            const Vec8 g = vec_load8<Tag>(drows + (((p.b * Ho + i) * Wo + j) * 9 + ky * 3 + kx) * (int64_t)C + p.c8 * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc.v[e] += g.v[e];
        }
    }
    vec_store8<Tag>(dx + it * 8, acc);
}

// y [B, 2H, 2W, C] <- x [B, H, W, C]
template <typename Tag>
__global__ __launch_bounds__(256) void upsample2_kernel(const typename Tag::storage* __restrict__ x, typename Tag::storage* __restrict__ y, int H, int W,
                                                        int C, int64_t items) {
    const int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (it >= items) return;
    const CsIdx p = cs_idx(it, 2 * H, 2 * W, C / 8);
    vec_store8<Tag>(y + it * 8, vec_load8<Tag>(x + ((p.b * H + p.y / 2) * W + p.x / 2) * (int64_t)C + p.c8 * 8));
}

// dx [B, H, W, C] <- dy [B, 2H, 2W, C]: ((00 + 01) + 10) + 11 in fp32
template <typename Tag>
__global__ __launch_bounds__(256) void upsample2_bwd_kernel(const typename Tag::storage* __restrict__ dy, typename Tag::storage* __restrict__ dx, int H,
                                                            int W, int C, int64_t items) {
    const int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (it >= items) return;
    const CsIdx p = cs_idx(it, H, W, C / 8);
    const typename Tag::storage* base = dy + ((p.b * 2 * H + 2 * p.y) * (2 * (int64_t)W) + 2 * p.x) * C + p.c8 * 8;
    Vec8 acc = vec_load8<Tag>(base);
    const Vec8 g01 = vec_load8<Tag>(base + C), g10 = vec_load8<Tag>(base + 2 * (int64_t)W * C), g11 = vec_load8<Tag>(base + 2 * (int64_t)W * C + C);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc.v[e] = ((acc.v[e] + g01.v[e]) + g10.v[e]) + g11.v[e];
    vec_store8<Tag>(dx + it * 8, acc);
}

// ---- row softmax -------------------------------------------------------------------------------------------------------------------
#define SM_THREADS 256
#define SM_SLOTS 2           // 8-column vectors a thread keeps in registers: rows of up to 256 * 2 * 8 = 4096 columns are read once

// eight consecutive columns [c, c + 8) of a row, columns >= n read as `fill`; VEC: one aligned vector access
template <typename Tag, bool VEC>
__device__ __forceinline__ Vec8 sm_load(const typename Tag::storage* row, int64_t c, int64_t n, float fill) {
    Vec8 v;
    if (VEC) {
        v = vec_load8<Tag>(row + c);
#pragma unroll
        for (int e = 0; e < 8; ++e) v.v[e] = c + e < n ? v.v[e] : fill;
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) v.v[e] = c + e < n ? Tag::load(row + c + e) : fill;
    }
    return v;
}
// store columns [c, c + 8) below ld
template <typename Tag, bool VEC>
__device__ __forceinline__ void sm_store(typename Tag::storage* row, int64_t c, int64_t ld, const Vec8& v) {
    if (VEC) vec_store8<Tag>(row + c, v);
    else {
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (c + e < ld) Tag::store(row + c + e, v.v[e]);
    }
}

// workgroup reductions in a fixed order: xor butterfly inside a wave, then the four wave results in wave order
template <bool MAX>
__device__ __forceinline__ float sm_block_reduce(float v, float* s_red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float w = __shfl_xor(v, o, 64);
        v = MAX ? fmaxf(v, w) : v + w;
    }
    __syncthreads();          // (s_red may still be read from the previous reduction)
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    return MAX ? fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3])) : ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
}

template <typename Tag, bool VEC>
__global__ __launch_bounds__(SM_THREADS) void softmax_rows_kernel(const float* __restrict__ S, int64_t lds, typename Tag::storage* __restrict__ P,
                                                                  int64_t ldp, int64_t N, float scale) {
    __shared__ float s_red[4];
    const int tid = threadIdx.x;
    const float* s = S + (int64_t)blockIdx.x * lds;
    typename Tag::storage* p = P + (int64_t)blockIdx.x * ldp;
    const float NEG = -3.0e38f;
    Vec8 c[SM_SLOTS];
    float m = NEG;
#pragma unroll
    for (int k = 0; k < SM_SLOTS; ++k) {
        const int64_t col = ((int64_t)k * SM_THREADS + tid) * 8;
        if (col < N) {
            c[k] = sm_load<F32Tag, VEC>(s, col, N, 0.f);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                c[k].v[e] = col + e < N ? c[k].v[e] * scale : NEG;
                m = fmaxf(m, c[k].v[e]);
            }
        }
    }
    for (int64_t col = ((int64_t)SM_SLOTS * SM_THREADS + tid) * 8; col < N; col += SM_THREADS * 8) {
        const Vec8 v = sm_load<F32Tag, VEC>(s, col, N, 0.f);
#pragma unroll
        for (int e = 0; e < 8; ++e) m = fmaxf(m, col + e < N ? v.v[e] * scale : NEG);
    }
    m = sm_block_reduce<true>(m, s_red);
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < SM_SLOTS; ++k) {
        const int64_t col = ((int64_t)k * SM_THREADS + tid) * 8;
        if (col < N) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                c[k].v[e] = col + e < N ? expf(c[k].v[e] - m) : 0.f;
                sum += c[k].v[e];
            }
        }
    }
    for (int64_t col = ((int64_t)SM_SLOTS * SM_THREADS + tid) * 8; col < N; col += SM_THREADS * 8) {
        const Vec8 v = sm_load<F32Tag, VEC>(s, col, N, 0.f);
#pragma unroll
        for (int e = 0; e < 8; ++e) sum += col + e < N ? expf(v.v[e] * scale - m) : 0.f;
    }
    sum = sm_block_reduce<false>(sum, s_red);
    const float inv = 1.f / sum;
#pragma unroll
    for (int k = 0; k < SM_SLOTS; ++k) {
        const int64_t col = ((int64_t)k * SM_THREADS + tid) * 8;
        if (col < ldp) {
            Vec8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o.v[e] = col + e < N ? c[k].v[e] * inv : 0.f;
            sm_store<Tag, VEC>(p, col, ldp, o);
        }
    }
    for (int64_t col = ((int64_t)SM_SLOTS * SM_THREADS + tid) * 8; col < ldp; col += SM_THREADS * 8) {
        Vec8 o = vec_zero8();
        if (col < N) {
            const Vec8 v = sm_load<F32Tag, VEC>(s, col, N, 0.f);
#pragma unroll
            for (int e = 0; e < 8; ++e) o.v[e] = col + e < N ? expf(v.v[e] * scale - m) * inv : 0.f;
        }
        sm_store<Tag, VEC>(p, col, ldp, o);
    }
}

// dS = scale P (dP - sum dP P); columns [N, ldp) = 0
template <typename Tag, bool VEC>
__global__ __launch_bounds__(SM_THREADS) void softmax_rows_bwd_kernel(const typename Tag::storage* __restrict__ P, const float* __restrict__ dP, int64_t lds,
                                                                      typename Tag::storage* __restrict__ dS, int64_t ldp, int64_t N, float scale) {
    __shared__ float s_red[4];
    const int tid = threadIdx.x;
    const typename Tag::storage* p = P + (int64_t)blockIdx.x * ldp;
    const float* g = dP + (int64_t)blockIdx.x * lds;
    typename Tag::storage* d = dS + (int64_t)blockIdx.x * ldp;
    Vec8 cp[SM_SLOTS], cg[SM_SLOTS];
    float dot = 0.f;
#pragma unroll
    for (int k = 0; k < SM_SLOTS; ++k) {
        const int64_t col = ((int64_t)k * SM_THREADS + tid) * 8;
        if (col < N) {
            cp[k] = sm_load<Tag, VEC>(p, col, N, 0.f);
            cg[k] = sm_load<F32Tag, VEC>(g, col, N, 0.f);
#pragma unroll
            for (int e = 0; e < 8; ++e) dot = fmaf(cp[k].v[e], cg[k].v[e], dot);
        }
    }
    for (int64_t col = ((int64_t)SM_SLOTS * SM_THREADS + tid) * 8; col < N; col += SM_THREADS * 8) {
        const Vec8 pv = sm_load<Tag, VEC>(p, col, N, 0.f), gv = sm_load<F32Tag, VEC>(g, col, N, 0.f);
#pragma unroll
        for (int e = 0; e < 8; ++e) dot = fmaf(pv.v[e], gv.v[e], dot);
    }
    dot = sm_block_reduce<false>(dot, s_red);
#pragma unroll
    for (int k = 0; k < SM_SLOTS; ++k) {
        const int64_t col = ((int64_t)k * SM_THREADS + tid) * 8;
        if (col < ldp) {
            Vec8 o = vec_zero8();
            if (col < N) {
#pragma unroll
                for (int e = 0; e < 8; ++e) o.v[e] = scale * cp[k].v[e] * (cg[k].v[e] - dot);       // (cp is 0 beyond N)
            }
            sm_store<Tag, VEC>(d, col, ldp, o);
        }
    }
    for (int64_t col = ((int64_t)SM_SLOTS * SM_THREADS + tid) * 8; col < ldp; col += SM_THREADS * 8) {
        Vec8 o = vec_zero8();
        if (col < N) {
            const Vec8 pv = sm_load<Tag, VEC>(p, col, N, 0.f), gv = sm_load<F32Tag, VEC>(g, col, N, 0.f);
#pragma unroll
            for (int e = 0; e < 8; ++e) o.v[e] = scale * pv.v[e] * (gv.v[e] - dot);
        }
        sm_store<Tag, VEC>(d, col, ldp, o);
    }
}

// ---- entry points ----------------------------------------------------------------------------------------------------------------
#define CS_GRID(items) dim3((unsigned)(((items) + 255) / 256))

static int haar_check(const char* fn, const void* img, const void* rows, int dtype, int B, int C, int H, int W, int ld, float scale) {
    UC_REQUIRE(img && rows, "%s: null pointer", fn);
    UC_REQUIRE_DTYPE(fn, dtype, true);
    UC_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, "%s: bad shape B=%d C=%d H=%d W=%d", fn, B, C, H, W);
    UC_REQUIRE(H % 4 == 0 && W % 4 == 0, "%s: H (%d) and W (%d) must be multiples of 4 (two Haar levels)", fn, H, W);
    UC_REQUIRE(C <= 4096 && ld >= 16 * C && ld % 8 == 0, "%s: ld (%d) must be a multiple of 8 and at least 16 C = %d (C <= 4096)", fn, ld, 16 * C);
    UC_REQUIRE(scale == scale && scale != 0.f, "%s: scale must be a non-zero number", fn);
    UC_REQUIRE((uintptr_t)img % 16 == 0 && (uintptr_t)rows % 16 == 0, "%s: img and rows must be 16-byte aligned", fn);
    UC_REQUIRE(((int64_t)B * C * (H / 4) * (W / 4) + 255) / 256 <= 0x7fffffff, "%s: grid limit exceeded", fn);
    return UC_OK;
}

extern "C" int uc_haar_patch(const float* img, void* rows, int dtype, int B, int C, int H, int W, int ld, float scale, uc_stream_t stream) {
    const char* fn = "uc_haar_patch";
    if (int e = haar_check(fn, img, rows, dtype, B, C, H, W, ld, scale)) return e;
    const int64_t items = (int64_t)B * C * (H / 4) * (W / 4);
    UC_DISPATCH_F16(fn, dtype, hipLaunchKernelGGL(haar_patch_kernel<Tag>, CS_GRID(items), dim3(256), 0, (hipStream_t)stream, img, (Tag::storage*)rows, C, H, W, ld, scale, items));
    UC_CHECK_LAUNCH(fn);
    return UC_OK;
}

extern "C" int uc_haar_unpatch(const void* rows, int dtype, float* img, int B, int C, int H, int W, int ld, float scale, uc_stream_t stream) {
    const char* fn = "uc_haar_unpatch";
    if (int e = haar_check(fn, img, rows, dtype, B, C, H, W, ld, scale)) return e;
    const int64_t items = (int64_t)B * C * (H / 4) * (W / 4);
    UC_DISPATCH_F16(fn, dtype, hipLaunchKernelGGL(haar_unpatch_kernel<Tag>, CS_GRID(items), dim3(256), 0, (hipStream_t)stream, (const Tag::storage*)rows, img, C, H, W, ld, scale, items));
    UC_CHECK_LAUNCH(fn);
    return UC_OK;
}

// `big`: the larger of the two maps, in 8-channel items (it bounds the grid and every index)
static int cs_check(const char* fn, const void* a, const void* b, int dtype, int B, int H, int W, int C, int64_t big) {
    UC_REQUIRE(a && b, "%s: null pointer", fn);
    UC_REQUIRE_DTYPE(fn, dtype, true);
    UC_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0, "%s: bad shape B=%d H=%d W=%d C=%d (C must be a multiple of 8)", fn, B, H, W, C);
    UC_REQUIRE((uintptr_t)a % 16 == 0 && (uintptr_t)b % 16 == 0, "%s: maps must be 16-byte aligned", fn);
    UC_REQUIRE(H <= 0x3ffffff0 && W <= 0x3ffffff0 && (big + 255) / 256 <= 0x7fffffff, "%s: grid limit exceeded", fn);
    return UC_OK;
}

extern "C" int uc_down2_gather(const void* x, void* rows, int dtype, int B, int H, int W, int C, uc_stream_t stream) {
    const char* fn = "uc_down2_gather";
    const int64_t items = (int64_t)B * (H / 2) * (W / 2) * 9 * (C / 8);
    if (int e = cs_check(fn, x, rows, dtype, B, H, W, C, items)) return e;
    UC_REQUIRE(H % 2 == 0 && W % 2 == 0, "%s: H (%d) and W (%d) must be even (the Downsample of an odd map has no HIP path)", fn, H, W);
    UC_DISPATCH_F16(fn, dtype, hipLaunchKernelGGL(down2_gather_kernel<Tag>, CS_GRID(items), dim3(256), 0, (hipStream_t)stream, (const Tag::storage*)x, (Tag::storage*)rows, H, W, C, items));
    UC_CHECK_LAUNCH(fn);
    return UC_OK;
}

extern "C" int uc_down2_gather_bwd(const void* drows, void* dx, int dtype, int B, int H, int W, int C, uc_stream_t stream) {
    const char* fn = "uc_down2_gather_bwd";
    const int64_t items = (int64_t)B * H * W * (C / 8);
    if (int e = cs_check(fn, drows, dx, dtype, B, H, W, C, (int64_t)B * (H / 2) * (W / 2) * 9 * (C / 8) + items)) return e;
    UC_REQUIRE(H % 2 == 0 && W % 2 == 0, "%s: H (%d) and W (%d) must be even (the Downsample of an odd map has no HIP path)", fn, H, W);
    UC_DISPATCH_F16(fn, dtype, hipLaunchKernelGGL(down2_gather_bwd_kernel<Tag>, CS_GRID(items), dim3(256), 0, (hipStream_t)stream, (const Tag::storage*)drows, (Tag::storage*)dx, H, W, C, items));
    UC_CHECK_LAUNCH(fn);
    return UC_OK;
}

extern "C" int uc_upsample2_nhwc(const void* x, void* y, int dtype, int B, int H, int W, int C, uc_stream_t stream) {
    const char* fn = "uc_upsample2_nhwc";
    const int64_t items = (int64_t)B * H * W * 4 * (C / 8);
    if (int e = cs_check(fn, x, y, dtype, B, H, W, C, items)) return e;
    UC_DISPATCH_F16(fn, dtype, hipLaunchKernelGGL(upsample2_kernel<Tag>, CS_GRID(items), dim3(256), 0, (hipStream_t)stream, (const Tag::storage*)x, (Tag::storage*)y, H, W, C, items));
    UC_CHECK_LAUNCH(fn);
    return UC_OK;
}

extern "C" int uc_upsample2_nhwc_bwd(const void* dy, void* dx, int dtype, int B, int H, int W, int C, uc_stream_t stream) {
    const char* fn = "uc_upsample2_nhwc_bwd";
    const int64_t items = (int64_t)B * H * W * (C / 8);
    if (int e = cs_check(fn, dy, dx, dtype, B, H, W, C, items * 4)) return e;
    UC_DISPATCH_F16(fn, dtype, hipLaunchKernelGGL(upsample2_bwd_kernel<Tag>, CS_GRID(items), dim3(256), 0, (hipStream_t)stream, (const Tag::storage*)dy, (Tag::storage*)dx, H, W, C, items));
    UC_CHECK_LAUNCH(fn);
    return UC_OK;
}

static int sm_check(const char* fn, const void* a, const void* b, const void* c, int dtype, int64_t lds, int64_t ldp, int64_t rows, int64_t N, float scale) {
    UC_REQUIRE(a && b && c, "%s: null pointer", fn);
    UC_REQUIRE_DTYPE(fn, dtype, true);
    UC_REQUIRE(rows > 0 && N > 0 && rows <= 0x7fffffff && N <= 0x7fffffff, "%s: bad shape rows=%lld N=%lld", fn, (long long)rows, (long long)N);
    UC_REQUIRE(lds >= N && ldp >= N && ldp <= 0x7fffffff, "%s: leading dimensions lds=%lld ldp=%lld must be at least N=%lld", fn, (long long)lds, (long long)ldp, (long long)N);
    UC_REQUIRE(scale == scale, "%s: scale is NaN", fn);
    UC_REQUIRE((uintptr_t)a % 4 == 0 && (uintptr_t)b % 4 == 0 && (uintptr_t)c % 4 == 0, "%s: misaligned pointer", fn);
    return UC_OK;
}
// 16-byte accesses: whole vectors stay inside a row's leading dimension and every row base is 16-byte aligned
#define SM_VEC(lds, ldp, a, b, c) ((lds) % 8 == 0 && (ldp) % 8 == 0 && (uintptr_t)(a) % 16 == 0 && (uintptr_t)(b) % 16 == 0 && (uintptr_t)(c) % 16 == 0)

extern "C" int uc_softmax_rows(const float* S, int64_t lds, void* P, int p_dtype, int64_t ldp, int64_t rows, int64_t N, float scale, uc_stream_t stream) {
    const char* fn = "uc_softmax_rows";
    if (int e = sm_check(fn, S, P, P, p_dtype, lds, ldp, rows, N, scale)) return e;
    hipStream_t st = (hipStream_t)stream;
    if (SM_VEC(lds, ldp, S, P, P))
        UC_DISPATCH_F16(fn, p_dtype, hipLaunchKernelGGL((softmax_rows_kernel<Tag, true>), dim3((unsigned)rows), dim3(SM_THREADS), 0, st, S, lds, (Tag::storage*)P, ldp, N, scale));
    else
        UC_DISPATCH_F16(fn, p_dtype, hipLaunchKernelGGL((softmax_rows_kernel<Tag, false>), dim3((unsigned)rows), dim3(SM_THREADS), 0, st, S, lds, (Tag::storage*)P, ldp, N, scale));
    UC_CHECK_LAUNCH(fn);
    return UC_OK;
}

extern "C" int uc_softmax_rows_bwd(const void* P, const float* dP, int64_t lds, void* dS, int p_dtype, int64_t ldp, int64_t rows, int64_t N, float scale,
                                   uc_stream_t stream) {
    const char* fn = "uc_softmax_rows_bwd";
    if (int e = sm_check(fn, P, dP, dS, p_dtype, lds, ldp, rows, N, scale)) return e;
    hipStream_t st = (hipStream_t)stream;
    if (SM_VEC(lds, ldp, P, dP, dS))
        UC_DISPATCH_F16(fn, p_dtype, hipLaunchKernelGGL((softmax_rows_bwd_kernel<Tag, true>), dim3((unsigned)rows), dim3(SM_THREADS), 0, st, (const Tag::storage*)P, dP, lds, (Tag::storage*)dS, ldp, N, scale));
    else
        UC_DISPATCH_F16(fn, p_dtype, hipLaunchKernelGGL((softmax_rows_bwd_kernel<Tag, false>), dim3((unsigned)rows), dim3(SM_THREADS), 0, st, (const Tag::storage*)P, dP, lds, (Tag::storage*)dS, ldp, N, scale));
    UC_CHECK_LAUNCH(fn);
    return UC_OK;
}
