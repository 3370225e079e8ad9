// GroupNorm on channels-last maps (the ResidualConvBlocks of the MoGe head: nn.GroupNorm + ReLU in front of every 3x3 convolution)
// and its backward.  x [B, H, W, C], G groups of C / G contiguous channels, (C / G) % 8 == 0.  The SiLU entry points (the Cosmos
// tokenizer's Normalize(128): 32 groups of 4) also take C / G == 4: a work item then spans two groups, its low and its high half.
//
// Work item = 8 consecutive channels of one pixel (vec_access.h).  A workgroup of 256 threads is laid out as `rows` pixels x C / 8
// channel vectors (rows = 256 / (C / 8)), so consecutive lanes read consecutive 16-byte pieces: a wave load covers whole pixel rows.
// One workgroup takes one CHUNK of rows * GN_VECS pixels of one sample — B x G alone would be a handful of workgroups.
//
//   forward statistics: a thread keeps its GN_VECS vectors in registers; the workgroup forms the chunk's sum per group, from it the
//     chunk mean, then the squared deviations from THAT mean (a true two-pass over registers: nothing cancels) and stores
//     (mean, M2) per (sample, chunk, group).  gn_stats_finalize merges the chunks with Chan's formula: one wave per (sample, group),
//     a lane merges chunks lane, lane + 64, ... in ascending order, the lanes are merged in a fixed butterfly.  No atomics.
//   apply: y = act((x - mean) rstd gamma + beta), a second kernel; act = none | ReLU | SiLU (the Cosmos tokenizer's Normalize + swish).
//   backward: per (sample, chunk, channel) partials of sum g x^ and sum g (g = dy, gated by y > 0 under a fused ReLU, times silu'(z)
//     with z recomputed from x under a fused SiLU); a per-sample
//     kernel adds the chunks in a fixed order (four interleaved chains, combined in chain order) and forms the two group sums
//     sum g gamma and sum g gamma x^ from the per-channel sums (they are gamma-weighted sums of those); a third adds the samples for
//     dgamma / dbeta; the fourth writes dx.  Fixed order everywhere: two calls give the same bits.
// The geometry (GnGeom, gn_geom, gn_group), the constants and the one shape rule live in groupnorm_plan.h, which the host compiler builds too.
#include "vec_access.h"
#include "groupnorm_plan.h"

// ---- workgroup reduction: per-thread value -> per-group value (threads are (row, channel vector); a group is cg8 adjacent vectors).
// Fixed order: rows ascending, then vectors ascending.  Result in s_grp[0..G); the caller synchronises before reading it.
__device__ __forceinline__ void gn_group_reduce(float val, float* s_thr, float* s_col, float* s_grp, int tid, int C8, int rows, int cg8, int G) {
    s_thr[tid] = val;
    __syncthreads();
    if (tid < C8) {
        float t = 0.f;
        for (int r = 0; r < rows; ++r) t += s_thr[r * C8 + tid];
        s_col[tid] = t;
    }
    __syncthreads();
    if (tid < G) {
        float t = 0.f;
        for (int k = 0; k < cg8; ++k) t += s_col[tid * cg8 + k];
        s_grp[tid] = t;
    }
    __syncthreads();
}

// grid (chunk, sample); part [B][nchunk][G] (mean, M2) of the chunk's valid pixels
template <typename Tag>
__global__ __launch_bounds__(GN_THREADS) void gn_stats_partial_kernel(const typename Tag::storage* __restrict__ x, float2* __restrict__ part,
                                                                      GnGeom gm) {
    __shared__ float s_thr[GN_THREADS], s_col[GN_THREADS], s_sum[GN_THREADS], s_m2[GN_THREADS];
    const int tid = threadIdx.x;
    const int C8 = gm.C8, rows = gm.rows;
    const bool active = tid < rows * C8;
    const int r = tid / C8, c8 = tid - r * C8;
    const int chunk = blockIdx.x;
    const int64_t b = blockIdx.y;
    const int p0 = chunk * gm.chunk_pix;
    const int npix = min(gm.chunk_pix, gm.HW - p0);
    const typename Tag::storage* base = x + ((b * gm.HW + p0) * (int64_t)gm.C) + c8 * 8;
    Vec8 v[GN_VECS];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < GN_VECS; ++j) {
        const int p = j * rows + r;
        if (active && p < npix) {
            v[j] = vec_load8<Tag>(base + (int64_t)p * gm.C);
#pragma unroll
            for (int e = 0; e < 8; ++e) s += v[j].v[e];
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[j].v[e] = 0.f;
        }
    }
    gn_group_reduce(active ? s : 0.f, s_thr, s_col, s_sum, tid, C8, rows, gm.cg8, gm.G);
    const float cnt = (float)npix * (float)(gm.cg8 * 8);
    const float mean = active ? s_sum[c8 / gm.cg8] / cnt : 0.f;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < GN_VECS; ++j) {
        const int p = j * rows + r;
        if (active && p < npix) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float d = v[j].v[e] - mean;
                q = fmaf(d, d, q);
            }
        }
    }
    gn_group_reduce(active ? q : 0.f, s_thr, s_col, s_m2, tid, C8, rows, gm.cg8, gm.G);
    if (tid < gm.G) part[(b * gm.nchunk + chunk) * gm.G + tid] = make_float2(s_sum[tid] / cnt, s_m2[tid]);
}

// the same for groups of 4 channels (gm.half): the workgroup reduction runs once per half, over single channel vectors
template <typename Tag>
__global__ __launch_bounds__(GN_THREADS) void gn_stats_partial4_kernel(const typename Tag::storage* __restrict__ x, float2* __restrict__ part,
                                                                       GnGeom gm) {
    __shared__ float s_thr[GN_THREADS], s_col[GN_THREADS], s_sum[2][GN_THREADS], s_m2[2][GN_THREADS];
    const int tid = threadIdx.x;
    const int C8 = gm.C8, rows = gm.rows;
    const bool active = tid < rows * C8;
    const int r = tid / C8, c8 = tid - r * C8;
    const int chunk = blockIdx.x;
    const int64_t b = blockIdx.y;
    const int p0 = chunk * gm.chunk_pix;
    const int npix = min(gm.chunk_pix, gm.HW - p0);
    const typename Tag::storage* base = x + ((b * gm.HW + p0) * (int64_t)gm.C) + c8 * 8;
    Vec8 v[GN_VECS];
    float s[2] = {0.f, 0.f};
#pragma unroll
    for (int j = 0; j < GN_VECS; ++j) {
        const int p = j * rows + r;
        if (active && p < npix) {
            v[j] = vec_load8<Tag>(base + (int64_t)p * gm.C);
#pragma unroll
            for (int e = 0; e < 8; ++e) s[e >> 2] += v[j].v[e];
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[j].v[e] = 0.f;
        }
    }
    const float cnt = (float)npix * 4.f;
    float mean[2], q[2] = {0.f, 0.f};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        gn_group_reduce(active ? s[h] : 0.f, s_thr, s_col, s_sum[h], tid, C8, rows, 1, C8);
        mean[h] = active ? s_sum[h][c8] / cnt : 0.f;
    }
#pragma unroll
    for (int j = 0; j < GN_VECS; ++j) {
        const int p = j * rows + r;
        if (active && p < npix) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float d = v[j].v[e] - mean[e >> 2];
                q[e >> 2] = fmaf(d, d, q[e >> 2]);
            }
        }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) gn_group_reduce(active ? q[h] : 0.f, s_thr, s_col, s_m2[h], tid, C8, rows, 1, C8);
    for (int g = tid; g < gm.G; g += GN_THREADS) part[(b * gm.nchunk + chunk) * gm.G + g] = make_float2(s_sum[g & 1][g >> 1] / cnt, s_m2[g & 1][g >> 1]);
}

// Chan et al.: (na, ma, Ma) + (nb, mb, Mb).  The element counts are carried in double: exact for any map the grid limits admit
// (a float count is inexact above 2^24 elements per (sample, group), e.g. 518 x 518 x 64 with G = 1).
__device__ __forceinline__ void gn_merge(double& na, float& ma, float& Ma, double nb, float mb, float Mb) {
    const double n = na + nb;
    const float f = n > 0.0 ? (float)(nb / n) : 0.f;
    const float d = mb - ma;
    ma = ma + d * f;
    Ma = (Ma + Mb) + (d * d) * ((float)na * f);
    na = n;
}

// one wave per (sample, group)
__global__ __launch_bounds__(64) void gn_stats_finalize_kernel(const float2* __restrict__ part, float* __restrict__ mean, float* __restrict__ rstd,
                                                               GnGeom gm, float eps) {
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x / gm.G;
    const int g = blockIdx.x - (int)b * gm.G;
    const double cg = (double)gm.cg;
    double n = 0.0;
    float mu = 0.f, m2 = 0.f;
    for (int k = lane; k < gm.nchunk; k += 64) {
        const float2 p = part[(b * gm.nchunk + k) * gm.G + g];
        gn_merge(n, mu, m2, (double)min(gm.chunk_pix, gm.HW - k * gm.chunk_pix) * cg, p.x, p.y);
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double n2 = __shfl_xor(n, o, 64);
        const float mu2 = __shfl_xor(mu, o, 64), m22 = __shfl_xor(m2, o, 64);
        // the lower lane's triple is always the left operand: both partners compute the same bits
        double an = (lane & o) ? n2 : n;
        float amu = (lane & o) ? mu2 : mu, am2 = (lane & o) ? m22 : m2;
        const double bn = (lane & o) ? n : n2;
        const float bmu = (lane & o) ? mu : mu2, bm2 = (lane & o) ? m2 : m22;
        gn_merge(an, amu, am2, bn, bmu, bm2);
        n = an; mu = amu; m2 = am2;
    }
    if (lane == 0) {
        mean[blockIdx.x] = mu;
        rstd[blockIdx.x] = 1.0f / sqrtf((float)((double)m2 / n) + eps);
    }
}

enum { GN_ACT_NONE = 0, GN_ACT_RELU = 1, GN_ACT_SILU = 2 };

// silu'(z) = s (1 + z (1 - s)), s = sigmoid(z)
__device__ __forceinline__ float gn_silu_grad(float z) {
    const float sg = 1.f / (1.f + expf(-z));
    return sg * fmaf(z, 1.f - sg, 1.f);
}

// one thread per (pixel, 8 channels)
template <typename Tag, int ACT>
__global__ __launch_bounds__(256) void gn_apply_kernel(const typename Tag::storage* __restrict__ x, typename Tag::storage* __restrict__ y,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       const float* __restrict__ mean, const float* __restrict__ rstd, int64_t items,
                                                       int64_t per_sample, GnGeom gm) {
    const int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (it >= items) return;
    const int64_t b = it / per_sample;
    const int c8 = (int)((it - b * per_sample) % gm.C8);
    const int sg[2] = {(int)b * gm.G + gn_group(gm, c8, 0), (int)b * gm.G + gn_group(gm, c8, 1)};
    const float mu[2] = {mean[sg[0]], mean[sg[1]]}, rs[2] = {rstd[sg[0]], rstd[sg[1]]};
    const Vec8 ga = vec_load8<F32Tag>(gamma + c8 * 8), be = vec_load8<F32Tag>(beta + c8 * 8);
    const Vec8 v = vec_load8<Tag>(x + it * 8);
    Vec8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float t = fmaf((v.v[e] - mu[e >> 2]) * rs[e >> 2], ga.v[e], be.v[e]);
        o.v[e] = ACT == GN_ACT_RELU ? fmaxf(t, 0.f) : ACT == GN_ACT_SILU ? t / (1.f + expf(-t)) : t;
    }
    vec_store8<Tag>(y + it * 8, o);
}

// ---- backward --------------------------------------------------------------------------------------------------------------------
// grid (chunk, sample); part [B][nchunk][2][C]: [0] = sum g x^, [1] = sum g over the chunk's pixels, per channel
// ACT: GN_ACT_RELU gates dy by gate > 0 (gate = the forward's y); GN_ACT_SILU multiplies it by silu'(z), z from x, gamma, beta
template <typename Tag, int ACT>
__global__ __launch_bounds__(GN_THREADS) void gn_bwd_partial_kernel(const typename Tag::storage* __restrict__ dy,
                                                                    const typename Tag::storage* __restrict__ x,
                                                                    const typename Tag::storage* __restrict__ gate,
                                                                    const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                    const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                    float* __restrict__ part, GnGeom gm) {
    __shared__ float s[16][GN_THREADS];
    const int tid = threadIdx.x;
    const int C8 = gm.C8, rows = gm.rows;
    const bool active = tid < rows * C8;
    const int r = tid / C8, c8 = tid - r * C8;
    const int chunk = blockIdx.x;
    const int64_t b = blockIdx.y;
    const int p0 = chunk * gm.chunk_pix;
    const int npix = min(gm.chunk_pix, gm.HW - p0);
    float a[8], bs[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] = bs[e] = 0.f;
    if (active) {
        const int sg[2] = {(int)b * gm.G + gn_group(gm, c8, 0), (int)b * gm.G + gn_group(gm, c8, 1)};
        const float mu[2] = {mean[sg[0]], mean[sg[1]]}, rs[2] = {rstd[sg[0]], rstd[sg[1]]};
        const int64_t off = ((b * gm.HW + p0) * (int64_t)gm.C) + c8 * 8;
        Vec8 ga, be;
        if (ACT == GN_ACT_SILU) { ga = vec_load8<F32Tag>(gamma + c8 * 8); be = vec_load8<F32Tag>(beta + c8 * 8); }
#pragma unroll 4
        for (int j = 0; j < GN_VECS; ++j) {
            const int p = j * rows + r;
            if (p < npix) {
                const int64_t o = off + (int64_t)p * gm.C;
                Vec8 g = vec_load8<Tag>(dy + o);
                const Vec8 xv = vec_load8<Tag>(x + o);
                if (ACT == GN_ACT_RELU) {
                    const Vec8 yv = vec_load8<Tag>(gate + o);
#pragma unroll
                    for (int e = 0; e < 8; ++e) g.v[e] = yv.v[e] > 0.f ? g.v[e] : 0.f;
                }
                if (ACT == GN_ACT_SILU) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) g.v[e] *= gn_silu_grad(fmaf((xv.v[e] - mu[e >> 2]) * rs[e >> 2], ga.v[e], be.v[e]));
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    a[e] = fmaf(g.v[e], (xv.v[e] - mu[e >> 2]) * rs[e >> 2], a[e]);
                    bs[e] += g.v[e];
                }
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) { s[e][tid] = a[e]; s[8 + e][tid] = bs[e]; }
    __syncthreads();
    float* dst = part + (b * gm.nchunk + chunk) * 2 * (int64_t)gm.C;
    for (int i = tid; i < 16 * C8; i += GN_THREADS) {
        const int k = i / C8, c = i - k * C8;       // k = which (0: g x^, 1: g) * 8 + channel within the vector
        float t = 0.f;
        for (int rr = 0; rr < rows; ++rr) t += s[k][rr * C8 + c];
        dst[(k >> 3) * gm.C + c * 8 + (k & 7)] = t;
    }
}

// one workgroup per sample: pc [B][2][C] = the chunk partials added up; S [B][G][2] = (sum g gamma, sum g gamma x^) per group
__global__ __launch_bounds__(256) void gn_bwd_finalize_kernel(const float* __restrict__ part, const float* __restrict__ gamma,
                                                              float* __restrict__ pc, float* __restrict__ S, GnGeom gm) {
    __shared__ float red[4][2][64];
    __shared__ float gs[2][GN_MAX_C];
    const int tid = threadIdx.x, q = tid >> 6, cl = tid & 63;
    const int64_t b = blockIdx.x;
    const int C = gm.C;
    for (int c0 = 0; c0 < C; c0 += 64) {
        const int c = c0 + cl;
        float a0 = 0.f, a1 = 0.f;
        if (c < C) {
            const float* p = part + b * gm.nchunk * 2 * (int64_t)C + c;
#pragma unroll 4
            for (int k = q; k < gm.nchunk; k += 4) {
                a0 += p[(int64_t)k * 2 * C];
                a1 += p[(int64_t)k * 2 * C + C];
            }
        }
        red[q][0][cl] = a0;
        red[q][1][cl] = a1;
        __syncthreads();
        if (q == 0 && c < C) {
            const float t0 = ((red[0][0][cl] + red[1][0][cl]) + red[2][0][cl]) + red[3][0][cl];
            const float t1 = ((red[0][1][cl] + red[1][1][cl]) + red[2][1][cl]) + red[3][1][cl];
            pc[(b * 2 + 0) * C + c] = t0;
            pc[(b * 2 + 1) * C + c] = t1;
            const float ga = gamma[c];
            gs[0][c] = ga * t1;
            gs[1][c] = ga * t0;
        }
        __syncthreads();
    }
    const int cg = gm.cg;
    for (int g = tid; g < gm.G; g += 256) {
        float s1 = 0.f, s2 = 0.f;
        for (int k = 0; k < cg; ++k) { s1 += gs[0][g * cg + k]; s2 += gs[1][g * cg + k]; }
        S[(b * gm.G + g) * 2 + 0] = s1;
        S[(b * gm.G + g) * 2 + 1] = s2;
    }
}

// one thread per (which, channel): dgamma / dbeta = the per-sample sums added in sample order
__global__ __launch_bounds__(256) void gn_bwd_params_kernel(const float* __restrict__ pc, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                            int B, int C) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * C) return;
    const int which = i / C, c = i - which * C;
    float t = 0.f;
    for (int b = 0; b < B; ++b) t += pc[((int64_t)b * 2 + which) * C + c];
    (which ? dbeta : dgamma)[c] = t;
}

template <typename Tag, int ACT>
__global__ __launch_bounds__(256) void gn_bwd_apply_kernel(const typename Tag::storage* __restrict__ dy, const typename Tag::storage* __restrict__ x,
                                                           const typename Tag::storage* __restrict__ gate, const float* __restrict__ mean,
                                                           const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, const float* __restrict__ S, typename Tag::storage* __restrict__ dx, int64_t items,
                                                           int64_t per_sample, float inv_m, GnGeom gm) {
    const int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (it >= items) return;
    const int64_t b = it / per_sample;
    const int c8 = (int)((it - b * per_sample) % gm.C8);
    const int sg[2] = {(int)b * gm.G + gn_group(gm, c8, 0), (int)b * gm.G + gn_group(gm, c8, 1)};
    const float mu[2] = {mean[sg[0]], mean[sg[1]]}, rs[2] = {rstd[sg[0]], rstd[sg[1]]};
    const float s1[2] = {S[sg[0] * 2] * inv_m, S[sg[1] * 2] * inv_m}, s2[2] = {S[sg[0] * 2 + 1] * inv_m, S[sg[1] * 2 + 1] * inv_m};
    const Vec8 ga = vec_load8<F32Tag>(gamma + c8 * 8);
    Vec8 g = vec_load8<Tag>(dy + it * 8);
    const Vec8 xv = vec_load8<Tag>(x + it * 8);
    if (ACT == GN_ACT_RELU) {
        const Vec8 yv = vec_load8<Tag>(gate + it * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) g.v[e] = yv.v[e] > 0.f ? g.v[e] : 0.f;
    }
    if (ACT == GN_ACT_SILU) {
        const Vec8 be = vec_load8<F32Tag>(beta + c8 * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) g.v[e] *= gn_silu_grad(fmaf((xv.v[e] - mu[e >> 2]) * rs[e >> 2], ga.v[e], be.v[e]));
    }
    Vec8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float xh = (xv.v[e] - mu[e >> 2]) * rs[e >> 2];
        o.v[e] = rs[e >> 2] * ((g.v[e] * ga.v[e] - s1[e >> 2]) - xh * s2[e >> 2]);
    }
    vec_store8<Tag>(dx + it * 8, o);
}

// ---- entry points ----------------------------------------------------------------------------------------------------------------
// group4: groups of 4 channels are accepted too (the SiLU entry points)
static int gn_check_shape(const char* fn, int dtype, int B, int H, int W, int C, int G, bool group4 = false) {
    UC_REQUIRE_DTYPE(fn, dtype, true);
    const GnShape rule = gn_shape_rule(B, H, W, C, G, group4);      // the one rule of groupnorm_plan.h; here only its messages
    UC_REQUIRE(rule != GN_SHAPE_DIMS, "%s: bad shape B=%d H=%d W=%d C=%d G=%d", fn, B, H, W, C, G);
    UC_REQUIRE(rule != GN_SHAPE_C_MOD_G, "%s: C (%d) is not a multiple of G (%d)", fn, C, G);
    UC_REQUIRE(rule != GN_SHAPE_GROUP, "%s: channels per group (%d) must be a multiple of 8%s", fn, C / G, group4 ? " (or 4)" : "");
    UC_REQUIRE(rule != GN_SHAPE_C_MOD_8, "%s: bad shape B=%d H=%d W=%d C=%d G=%d (C must be a multiple of 8)", fn, B, H, W, C, G);
    UC_REQUIRE(rule != GN_SHAPE_MAX_C, "%s: C (%d) exceeds %d", fn, C, GN_MAX_C);
    UC_REQUIRE(rule != GN_SHAPE_GRID, "%s: grid limit exceeded (B <= 65535, H * W < 2^31, B * H * W * C < 2^42)", fn);
    return UC_OK;
}

static_assert(sizeof(float2) == 8, "gn_fwd_ws_bytes counts (mean, M2) as 8 bytes");

extern "C" int64_t uc_group_norm_nhwc_ws_bytes(int64_t B, int64_t H, int64_t W, int64_t C, int64_t G) {
    return gn_shape_ok(B, H, W, C, G, false) ? gn_fwd_ws_bytes(B, H, W, C, G) : 0;
}
extern "C" int64_t uc_group_norm_silu_nhwc_ws_bytes(int64_t B, int64_t H, int64_t W, int64_t C, int64_t G) {
    return gn_shape_ok(B, H, W, C, G, true) ? gn_fwd_ws_bytes(B, H, W, C, G) : 0;
}

static int gn_forward(const char* fn, const void* x, void* y, const float* gamma, const float* beta, float* mean, float* rstd, float* ws,
                      int dtype, int B, int H, int W, int C, int G, float eps, int act, uc_stream_t stream) {
    UC_REQUIRE(x && y && gamma && beta && mean && rstd && ws, "%s: null pointer", fn);
    if (int e = gn_check_shape(fn, dtype, B, H, W, C, G, act == GN_ACT_SILU)) return e;
    UC_REQUIRE(eps > 0.f, "%s: eps must be positive", fn);
    UC_REQUIRE((uintptr_t)x % 16 == 0 && (uintptr_t)y % 16 == 0 && (uintptr_t)gamma % 16 == 0 && (uintptr_t)beta % 16 == 0 &&
                   (uintptr_t)ws % 8 == 0 && (uintptr_t)mean % 4 == 0 && (uintptr_t)rstd % 4 == 0,
               "%s: x, y, gamma, beta must be 16-byte aligned (ws 8, mean / rstd 4)", fn);
    const GnGeom gm = gn_geom(H, W, C, G);
    hipStream_t st = (hipStream_t)stream;
    const dim3 pgrid((unsigned)gm.nchunk, (unsigned)B);
    if (gm.half)
        UC_DISPATCH_F16(fn, dtype, hipLaunchKernelGGL(gn_stats_partial4_kernel<Tag>, pgrid, dim3(GN_THREADS), 0, st, (const Tag::storage*)x, (float2*)ws, gm));
    else
        UC_DISPATCH_F16(fn, dtype, hipLaunchKernelGGL(gn_stats_partial_kernel<Tag>, pgrid, dim3(GN_THREADS), 0, st, (const Tag::storage*)x, (float2*)ws, gm));
    UC_CHECK_LAUNCH(fn);
    hipLaunchKernelGGL(gn_stats_finalize_kernel, dim3((unsigned)(B * G)), dim3(64), 0, st, (const float2*)ws, mean, rstd, gm, eps);
    UC_CHECK_LAUNCH(fn);
    const int64_t per_sample = (int64_t)gm.HW * gm.C8, items = per_sample * B;
    const dim3 agrid((unsigned)((items + 255) / 256));
    if (act == GN_ACT_SILU)
        UC_DISPATCH_F16(fn, dtype, hipLaunchKernelGGL((gn_apply_kernel<Tag, GN_ACT_SILU>), agrid, dim3(256), 0, st, (const Tag::storage*)x, (Tag::storage*)y, gamma, beta,
                                              (const float*)mean, (const float*)rstd, items, per_sample, gm));
    else if (act == GN_ACT_RELU)
        UC_DISPATCH_F16(fn, dtype, hipLaunchKernelGGL((gn_apply_kernel<Tag, GN_ACT_RELU>), agrid, dim3(256), 0, st, (const Tag::storage*)x, (Tag::storage*)y, gamma, beta,
                                              (const float*)mean, (const float*)rstd, items, per_sample, gm));
    else
        UC_DISPATCH_F16(fn, dtype, hipLaunchKernelGGL((gn_apply_kernel<Tag, GN_ACT_NONE>), agrid, dim3(256), 0, st, (const Tag::storage*)x, (Tag::storage*)y, gamma, beta,
                                              (const float*)mean, (const float*)rstd, items, per_sample, gm));
    UC_CHECK_LAUNCH(fn);
    return UC_OK;
}

extern "C" int uc_group_norm_nhwc(const void* x, void* y, const float* gamma, const float* beta, float* mean, float* rstd, float* ws,
                                  int dtype, int B, int H, int W, int C, int G, float eps, int relu, uc_stream_t stream) {
    return gn_forward("uc_group_norm_nhwc", x, y, gamma, beta, mean, rstd, ws, dtype, B, H, W, C, G, eps, relu ? GN_ACT_RELU : GN_ACT_NONE, stream);
}

extern "C" int uc_group_norm_silu_nhwc(const void* x, void* y, const float* gamma, const float* beta, float* mean, float* rstd, float* ws,
                                       int dtype, int B, int H, int W, int C, int G, float eps, uc_stream_t stream) {
    return gn_forward("uc_group_norm_silu_nhwc", x, y, gamma, beta, mean, rstd, ws, dtype, B, H, W, C, G, eps, GN_ACT_SILU, stream);
}

extern "C" int64_t uc_group_norm_nhwc_bwd_ws_bytes(int64_t B, int64_t H, int64_t W, int64_t C, int64_t G) {
    return gn_shape_ok(B, H, W, C, G, false) ? gn_bwd_ws_bytes(B, H, W, C, G) : 0;
}
extern "C" int64_t uc_group_norm_silu_nhwc_bwd_ws_bytes(int64_t B, int64_t H, int64_t W, int64_t C, int64_t G) {
    return gn_shape_ok(B, H, W, C, G, true) ? gn_bwd_ws_bytes(B, H, W, C, G) : 0;
}

// beta != NULL: the fused SiLU's backward (gate unused); gate != NULL: the fused ReLU's
static int gn_backward(const char* fn, const void* dy, const void* x, const void* gate, const float* mean, const float* rstd,
                       const float* gamma, const float* beta, void* dx, float* dgamma, float* dbeta, float* ws, int dtype, int B, int H, int W,
                       int C, int G, uc_stream_t stream) {
    UC_REQUIRE(dy && x && mean && rstd && gamma && dx && dgamma && dbeta && ws, "%s: null pointer", fn);
    UC_REQUIRE(!beta || (uintptr_t)beta % 16 == 0, "%s: beta must be 16-byte aligned", fn);
    if (int e = gn_check_shape(fn, dtype, B, H, W, C, G, beta != nullptr)) return e;
    UC_REQUIRE((uintptr_t)dy % 16 == 0 && (uintptr_t)x % 16 == 0 && (uintptr_t)dx % 16 == 0 && (uintptr_t)gamma % 16 == 0 &&
                   (!gate || (uintptr_t)gate % 16 == 0) && (uintptr_t)ws % 4 == 0 && (uintptr_t)dgamma % 4 == 0 && (uintptr_t)dbeta % 4 == 0 &&
                   (uintptr_t)mean % 4 == 0 && (uintptr_t)rstd % 4 == 0,
               "%s: dy, x, gate, dx, gamma must be 16-byte aligned (the fp32 vectors 4)", fn);
    const GnGeom gm = gn_geom(H, W, C, G);
    hipStream_t st = (hipStream_t)stream;
    float* part = ws;
    float* pc = part + (int64_t)B * gm.nchunk * 2 * C;
    float* S = pc + (int64_t)B * 2 * C;
    const dim3 pgrid((unsigned)gm.nchunk, (unsigned)B);
    if (beta)
        UC_DISPATCH_F16(fn, dtype, hipLaunchKernelGGL((gn_bwd_partial_kernel<Tag, GN_ACT_SILU>), pgrid, dim3(GN_THREADS), 0, st, (const Tag::storage*)dy, (const Tag::storage*)x,
                                              (const Tag::storage*)nullptr, mean, rstd, gamma, beta, part, gm));
    else if (gate)
        UC_DISPATCH_F16(fn, dtype, hipLaunchKernelGGL((gn_bwd_partial_kernel<Tag, GN_ACT_RELU>), pgrid, dim3(GN_THREADS), 0, st, (const Tag::storage*)dy, (const Tag::storage*)x,
                                              (const Tag::storage*)gate, mean, rstd, gamma, beta, part, gm));
    else
        UC_DISPATCH_F16(fn, dtype, hipLaunchKernelGGL((gn_bwd_partial_kernel<Tag, GN_ACT_NONE>), pgrid, dim3(GN_THREADS), 0, st, (const Tag::storage*)dy, (const Tag::storage*)x,
                                              (const Tag::storage*)nullptr, mean, rstd, gamma, beta, part, gm));
    UC_CHECK_LAUNCH(fn);
    hipLaunchKernelGGL(gn_bwd_finalize_kernel, dim3((unsigned)B), dim3(256), 0, st, (const float*)part, gamma, pc, S, gm);
    UC_CHECK_LAUNCH(fn);
    hipLaunchKernelGGL(gn_bwd_params_kernel, dim3((unsigned)((2 * C + 255) / 256)), dim3(256), 0, st, (const float*)pc, dgamma, dbeta, B, C);
    UC_CHECK_LAUNCH(fn);
    const int64_t per_sample = (int64_t)gm.HW * gm.C8, items = per_sample * B;
    const dim3 agrid((unsigned)((items + 255) / 256));
    const float inv_m = (float)(1.0 / ((double)gm.HW * (double)gm.cg));
    if (beta)
        UC_DISPATCH_F16(fn, dtype, hipLaunchKernelGGL((gn_bwd_apply_kernel<Tag, GN_ACT_SILU>), agrid, dim3(256), 0, st, (const Tag::storage*)dy, (const Tag::storage*)x,
                                              (const Tag::storage*)nullptr, mean, rstd, gamma, beta, (const float*)S, (Tag::storage*)dx, items, per_sample, inv_m, gm));
    else if (gate)
        UC_DISPATCH_F16(fn, dtype, hipLaunchKernelGGL((gn_bwd_apply_kernel<Tag, GN_ACT_RELU>), agrid, dim3(256), 0, st, (const Tag::storage*)dy, (const Tag::storage*)x, (const Tag::storage*)gate,
                                              mean, rstd, gamma, beta, (const float*)S, (Tag::storage*)dx, items, per_sample, inv_m, gm));
    else
        UC_DISPATCH_F16(fn, dtype, hipLaunchKernelGGL((gn_bwd_apply_kernel<Tag, GN_ACT_NONE>), agrid, dim3(256), 0, st, (const Tag::storage*)dy, (const Tag::storage*)x,
                                              (const Tag::storage*)nullptr, mean, rstd, gamma, beta, (const float*)S, (Tag::storage*)dx, items, per_sample, inv_m, gm));
    UC_CHECK_LAUNCH(fn);
    return UC_OK;
}

extern "C" int uc_group_norm_nhwc_bwd(const void* dy, const void* x, const void* gate, const float* mean, const float* rstd,
                                      const float* gamma, void* dx, float* dgamma, float* dbeta, float* ws, int dtype, int B, int H, int W,
                                      int C, int G, uc_stream_t stream) {
    return gn_backward("uc_group_norm_nhwc_bwd", dy, x, gate, mean, rstd, gamma, nullptr, dx, dgamma, dbeta, ws, dtype, B, H, W, C, G, stream);
}

extern "C" int uc_group_norm_silu_nhwc_bwd(const void* dy, const void* x, const float* mean, const float* rstd, const float* gamma,
                                           const float* beta, void* dx, float* dgamma, float* dbeta, float* ws, int dtype, int B, int H, int W,
                                           int C, int G, uc_stream_t stream) {
    const char* fn = "uc_group_norm_silu_nhwc_bwd";
    UC_REQUIRE(beta, "%s: null pointer", fn);
    return gn_backward(fn, dy, x, nullptr, mean, rstd, gamma, beta, dx, dgamma, dbeta, ws, dtype, B, H, W, C, G, stream);
}
