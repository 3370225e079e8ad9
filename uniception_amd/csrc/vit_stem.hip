// The stem of a ViT whose token assembly ends in a LayerNorm (gfx950), forward and backward:
//   z[b, t, :] = (t < ncls ? cls : tok[b, t - ncls, :]) + pos[t, :],     y = LN(z) gamma + beta,     T = hw + ncls, ncls = (cls != NULL)
// tok is the patch GEMM's output, y the residual stream.  One wavefront per row, the row in registers as chunks of eight channels
// per lane (C % 8 == 0, C <= 64 * 8 * VS_MAXV), statistics two-pass in fp32 (the mean first, the deviations from it second, as
// uc_ln_pe_ln).  Nothing here allocates; every output element is written once by a plain store and every sum runs in a fixed order
// (no atomics): the same bits on every run.
#include "vec_access.h"

#define VS_MAXV 4
#define VS_BSLAB 8      // images per wavefront of the backward: the first stage of dpos[t] = sum_b dz[b, t]
#define VS_TSLAB 8      // tokens per wavefront of the backward: with VS_BSLAB the first stage of dgamma / dbeta (64 rows)

// the lane's chunks of row (b, t) of z; cls / pos may be NULL (wave-uniform branches)
template <typename TT, int NI>
__device__ __forceinline__ void stem_row(Vec8 (&z)[NI], const typename TT::storage* __restrict__ tok, const float* __restrict__ cls,
                                         const float* __restrict__ pos, int64_t b, int t, int hw, int C, int lane) {
    const int ncls = cls ? 1 : 0;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int c = (i * 64 + lane) * 8;
        if (c < C) {
            z[i] = t < ncls ? vec_load8<F32Tag>(cls + c) : vec_load8<TT>(tok + (b * hw + (t - ncls)) * C + c);
            if (pos) {
                const Vec8 p = vec_load8<F32Tag>(pos + (int64_t)t * C + c);
#pragma unroll
                for (int j = 0; j < 8; ++j) z[i].v[j] += p.v[j];
            }
        }
    }
}

struct StemArgs {
    const float *cls, *pos, *gamma, *beta;
    float2* stats;
    float eps;
    int64_t rows;
    int T, hw, C;
};

template <typename TI, typename TO, int NI>
__global__ __launch_bounds__(256) void vit_stem_kernel(const typename TI::storage* __restrict__ tok, typename TO::storage* __restrict__ y, StemArgs a) {
    const int C = a.C;
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.rows) return;
    const int64_t b = row / a.T;
    const int t = (int)(row - b * a.T);
    Vec8 z[NI];
    stem_row<TI, NI>(z, tok, a.cls, a.pos, b, t, a.hw, C, lane);
    if (a.gamma) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < NI; ++i)
            if ((i * 64 + lane) * 8 < C)
                s += ((z[i].v[0] + z[i].v[1]) + (z[i].v[2] + z[i].v[3])) + ((z[i].v[4] + z[i].v[5]) + (z[i].v[6] + z[i].v[7]));
        const float mean = wave_sum(s) / (float)C;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < NI; ++i)
            if ((i * 64 + lane) * 8 < C) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    z[i].v[j] -= mean;
                    q += z[i].v[j] * z[i].v[j];
                }
            }
        const float rstd = rsqrtf(wave_sum(q) / (float)C + a.eps);
        if (a.stats && lane == 0) a.stats[row] = make_float2(mean, rstd);
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int c = (i * 64 + lane) * 8;
            if (c < C) {
                const Vec8 g = vec_load8<F32Tag>(a.gamma + c), bb = vec_load8<F32Tag>(a.beta + c);
#pragma unroll
                for (int j = 0; j < 8; ++j) z[i].v[j] = z[i].v[j] * rstd * g.v[j] + bb.v[j];
            }
        }
    }
    typename TO::storage* yr = y + row * C;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int c = (i * 64 + lane) * 8;
        if (c < C) vec_store8<TO>(yr + c, z[i]);
    }
}

// ---- backward --------------------------------------------------------------------------------------------------------------------------
// Wavefront (s, tg) walks the tokens [tg VS_TSLAB, +VS_TSLAB) and, per token, the images [s VS_BSLAB, +VS_BSLAB), both ascending:
// z is recomputed, dz = LN backward of dy (or dy itself without a norm) goes to dtok, the sum of dz over the wave's images to
// pos_part[s][t][C], the sums of dy x^ and dy over the wave's 64 rows to gb_part[s][tg][2][C].  The merge kernels add the partials
// with s (and tg) ascending.
struct StemBwdArgs {
    const float *cls, *pos, *gamma;
    const float2* stats;
    float *pos_part, *gb_part;
    int B, T, hw, C, S, TG;
};

template <typename TD, typename TT, int NI>
__global__ __launch_bounds__(256) void vit_stem_bwd_kernel(const typename TD::storage* __restrict__ dy, const typename TT::storage* __restrict__ tok,
                                                           typename TT::storage* __restrict__ dtok, StemBwdArgs a) {
    const int C = a.C;
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= (int64_t)a.S * a.TG) return;
    const int s = (int)(w / a.TG), tg = (int)(w - (int64_t)s * a.TG);
    const int ncls = a.cls ? 1 : 0;
    const float invC = 1.0f / (float)C;
    Vec8 gam[NI], dg[NI], db[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int c = (i * 64 + lane) * 8;
#pragma unroll
        for (int j = 0; j < 8; ++j) dg[i].v[j] = db[i].v[j] = gam[i].v[j] = 0.f;
        if (a.gamma && c < C) gam[i] = vec_load8<F32Tag>(a.gamma + c);
    }
    const int t1 = min(a.T, (tg + 1) * VS_TSLAB), b1 = min(a.B, (s + 1) * VS_BSLAB);
    for (int t = tg * VS_TSLAB; t < t1; ++t) {
        Vec8 dp[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) dp[i].v[j] = 0.f;
        for (int b = s * VS_BSLAB; b < b1; ++b) {
            const int64_t row = (int64_t)b * a.T + t;
            Vec8 g[NI];
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const int c = (i * 64 + lane) * 8;
                if (c < C) g[i] = vec_load8<TD>(dy + row * C + c);
            }
            if (a.gamma) {
                Vec8 z[NI];
                stem_row<TT, NI>(z, tok, a.cls, a.pos, b, t, a.hw, C, lane);
                const float2 st = a.stats[row];
                float s1 = 0.f, s2 = 0.f;
#pragma unroll
                for (int i = 0; i < NI; ++i)
                    if ((i * 64 + lane) * 8 < C) {
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            const float xh = (z[i].v[j] - st.x) * st.y;
                            z[i].v[j] = xh;
                            db[i].v[j] += g[i].v[j];
                            dg[i].v[j] += g[i].v[j] * xh;
                            g[i].v[j] *= gam[i].v[j];
                            s1 += g[i].v[j];
                            s2 += g[i].v[j] * xh;
                        }
                    }
                s1 = wave_sum(s1) * invC;
                s2 = wave_sum(s2) * invC;
#pragma unroll
                for (int i = 0; i < NI; ++i)
#pragma unroll
                    for (int j = 0; j < 8; ++j) g[i].v[j] = st.y * (g[i].v[j] - s1 - z[i].v[j] * s2);
            }
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const int c = (i * 64 + lane) * 8;
                if (c < C) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) dp[i].v[j] += g[i].v[j];
                    if (dtok && t >= ncls) vec_store8<TT>(dtok + ((int64_t)b * a.hw + (t - ncls)) * C + c, g[i]);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int c = (i * 64 + lane) * 8;
            if (c < C) vec_store8<F32Tag>(a.pos_part + ((int64_t)s * a.T + t) * C + c, dp[i]);
        }
    }
    if (a.gamma) {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int c = (i * 64 + lane) * 8;
            if (c < C) {
                vec_store8<F32Tag>(a.gb_part + (((int64_t)s * a.TG + tg) * 2 + 0) * C + c, dg[i]);
                vec_store8<F32Tag>(a.gb_part + (((int64_t)s * a.TG + tg) * 2 + 1) * C + c, db[i]);
            }
        }
    }
}

// dpos[t, c] = sum_s pos_part[s][t][c]; dcls = row 0 of that sum
__global__ __launch_bounds__(256) void vit_stem_merge_pos_kernel(const float* __restrict__ part, float* __restrict__ dpos, float* __restrict__ dcls, int S,
                                                                 int64_t TC, int C) {
    for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < TC; it += (int64_t)gridDim.x * 256) {
        float v = 0.f;
        for (int s = 0; s < S; ++s) v += part[s * TC + it];
        if (dpos) dpos[it] = v;
        if (dcls && it < C) dcls[it] = v;
    }
}

__global__ __launch_bounds__(256) void vit_stem_merge_gb_kernel(const float* __restrict__ part, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                                int64_t n, int C) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    float dg = 0.f, db = 0.f;
    for (int64_t i = 0; i < n; ++i) {
        dg += part[(i * 2 + 0) * C + c];
        db += part[(i * 2 + 1) * C + c];
    }
    if (dgamma) dgamma[c] = dg;
    if (dbeta) dbeta[c] = db;
}

// ---- entry points ----------------------------------------------------------------------------------------------------------------------
static int stem_check_shape(const char* fn, int64_t B, int64_t hw, int C) {
    UC_REQUIRE(B > 0 && hw > 0 && B <= 0x7fffffff && hw < 0x7fffffff && (B * (hw + 1) + 3) / 4 <= 0x7fffffff, "%s: bad shape B=%lld hw=%lld", fn,
               (long long)B, (long long)hw);
    UC_REQUIRE(C > 0 && C % 8 == 0 && C <= 64 * 8 * VS_MAXV, "%s: C=%d must be a multiple of 8, at most %d", fn, C, 64 * 8 * VS_MAXV);
    return UC_OK;
}

template <typename TI, typename TO>
static void stem_launch(const void* tok, void* y, const StemArgs& a, hipStream_t st) {
    typedef typename TI::storage SI;
    typedef typename TO::storage SO;
    const dim3 grid((unsigned)ceil_div64(a.rows, 4));
#define VS_FWD(NI_) hipLaunchKernelGGL((vit_stem_kernel<TI, TO, NI_>), grid, dim3(256), 0, st, (const SI*)tok, (SO*)y, a)
    if (a.C <= 512) VS_FWD(1);
    else if (a.C <= 1024) VS_FWD(2);
    else if (a.C <= 1536) VS_FWD(3);
    else VS_FWD(4);
#undef VS_FWD
}

template <typename TI>
static int stem_dispatch_out(const char* fn, const void* tok, void* y, int y_dtype, const StemArgs& a, hipStream_t st) {
    UC_DISPATCH(fn, y_dtype, (stem_launch<TI, Tag>(tok, y, a, st)));
    return UC_OK;
}

extern "C" int uc_vit_stem(const void* tok, int tok_dtype, const float* cls, const float* pos, const float* gamma, const float* beta, float eps, void* y,
                           int y_dtype, float* stats, int64_t B, int64_t hw, int C, uc_stream_t stream) {
    const char* fn = "uc_vit_stem";
    UC_REQUIRE_DTYPE(fn, tok_dtype, false);
    UC_REQUIRE_DTYPE(fn, y_dtype, false);
    UC_REQUIRE(tok && y, "%s: null pointer", fn);
    if (int e = stem_check_shape(fn, B, hw, C)) return e;
    UC_REQUIRE((gamma != nullptr) == (beta != nullptr), "%s: the norm takes gamma and beta together (both NULL: no LayerNorm)", fn);
    UC_REQUIRE(!gamma || eps > 0.f, "%s: eps must be positive (eps=%g)", fn, (double)eps);
    UC_REQUIRE(!stats || gamma, "%s: stats without a LayerNorm", fn);
    UC_REQUIRE(((uintptr_t)tok | (uintptr_t)y | (uintptr_t)cls | (uintptr_t)pos | (uintptr_t)gamma | (uintptr_t)beta) % 16 == 0 && (uintptr_t)stats % 8 == 0,
               "%s: tok, y, cls, pos, gamma and beta must be 16-byte aligned, stats 8-byte", fn);
    StemArgs a;
    a.cls = cls; a.pos = pos; a.gamma = gamma; a.beta = beta; a.stats = (float2*)stats; a.eps = eps;
    a.hw = (int)hw; a.T = (int)hw + (cls ? 1 : 0); a.rows = B * a.T; a.C = C;
    hipStream_t st = (hipStream_t)stream;
    if (int e = tok_dtype == UC_F32 ? stem_dispatch_out<F32Tag>(fn, tok, y, y_dtype, a, st) : stem_dispatch_out<BF16Tag>(fn, tok, y, y_dtype, a, st)) return e;
    UC_CHECK_LAUNCH(fn);
    return UC_OK;
}

extern "C" int64_t uc_vit_stem_ws_bytes(int64_t B, int64_t T, int64_t C) {
    if (B <= 0 || T <= 0 || C <= 0) return 0;
    const int64_t S = ceil_div64(B, VS_BSLAB), TG = ceil_div64(T, VS_TSLAB);
    return (int64_t)sizeof(float) * (S * T * C + S * TG * 2 * C);
}

template <typename TD, typename TT>
static void stem_bwd_launch(const void* dy, const void* tok, void* dtok, const StemBwdArgs& a, hipStream_t st) {
    typedef typename TD::storage SD;
    typedef typename TT::storage ST;
    const dim3 grid((unsigned)ceil_div64((int64_t)a.S * a.TG, 4));
#define VS_BWD(NI_) hipLaunchKernelGGL((vit_stem_bwd_kernel<TD, TT, NI_>), grid, dim3(256), 0, st, (const SD*)dy, (const ST*)tok, (ST*)dtok, a)
    if (a.C <= 512) VS_BWD(1);
    else if (a.C <= 1024) VS_BWD(2);
    else if (a.C <= 1536) VS_BWD(3);
    else VS_BWD(4);
#undef VS_BWD
}

template <typename TD>
static int stem_bwd_dispatch_tok(const char* fn, const void* dy, const void* tok, int tok_dtype, void* dtok, const StemBwdArgs& a, hipStream_t st) {
    UC_DISPATCH(fn, tok_dtype, (stem_bwd_launch<TD, Tag>(dy, tok, dtok, a, st)));
    return UC_OK;
}

extern "C" int uc_vit_stem_bwd(const void* dy, int dy_dtype, const void* tok, int tok_dtype, const float* cls, const float* pos, const float* gamma,
                               const float* stats, void* dtok, float* dcls, float* dpos, float* dgamma, float* dbeta, float* ws, int64_t B, int64_t hw,
                               int C, uc_stream_t stream) {
    const char* fn = "uc_vit_stem_bwd";
    UC_REQUIRE_DTYPE(fn, dy_dtype, false);
    UC_REQUIRE_DTYPE(fn, tok_dtype, false);
    UC_REQUIRE(dy && tok && ws, "%s: null pointer (dy, tok, ws)", fn);
    if (int e = stem_check_shape(fn, B, hw, C)) return e;
    UC_REQUIRE(!gamma || stats, "%s: the LayerNorm's backward needs the forward's stats", fn);
    UC_REQUIRE(gamma || (!dgamma && !dbeta), "%s: dgamma / dbeta without a LayerNorm", fn);
    UC_REQUIRE(cls || !dcls, "%s: dcls without a class token", fn);
    UC_REQUIRE(pos || !dpos, "%s: dpos without a position table", fn);
    UC_REQUIRE(((uintptr_t)dy | (uintptr_t)tok | (uintptr_t)dtok | (uintptr_t)cls | (uintptr_t)pos | (uintptr_t)gamma | (uintptr_t)ws) % 16 == 0 &&
                   (uintptr_t)stats % 8 == 0,
               "%s: dy, tok, dtok, cls, pos, gamma and ws must be 16-byte aligned, stats 8-byte", fn);
    StemBwdArgs a;
    a.cls = cls; a.pos = pos; a.gamma = gamma; a.stats = (const float2*)stats;
    a.B = (int)B; a.hw = (int)hw; a.T = (int)hw + (cls ? 1 : 0); a.C = C;
    a.S = (int)ceil_div64(B, VS_BSLAB); a.TG = (int)ceil_div64(a.T, VS_TSLAB);
    a.pos_part = ws;
    a.gb_part = ws + (int64_t)a.S * a.T * C;
    hipStream_t st = (hipStream_t)stream;
    if (int e = dy_dtype == UC_F32 ? stem_bwd_dispatch_tok<F32Tag>(fn, dy, tok, tok_dtype, dtok, a, st)
                                   : stem_bwd_dispatch_tok<BF16Tag>(fn, dy, tok, tok_dtype, dtok, a, st)) return e;
    if (dpos || dcls) {
        const int64_t TC = (int64_t)a.T * C;
        hipLaunchKernelGGL(vit_stem_merge_pos_kernel, dim3(EW_GRID(TC)), dim3(256), 0, st, a.pos_part, dpos, dcls, a.S, TC, C);
    }
    if (dgamma || dbeta)
        hipLaunchKernelGGL(vit_stem_merge_gb_kernel, dim3((unsigned)ceil_div64(C, 256)), dim3(256), 0, st, a.gb_part, dgamma, dbeta, (int64_t)a.S * a.TG, C);
    UC_CHECK_LAUNCH(fn);
    return UC_OK;
}
