// Streaming steps of the non-image input encoders (gfx950): PixelUnshuffle as GEMM operand rows and its adjoint, the activation that
// follows a residual sum, and LN2(LN1(x) + pe) in one pass over the token rows.  Nothing here allocates; every output element is
// written once by a plain store and every reduction (the row statistics) runs in a fixed order: the same bits on every run.
#include "vec_access.h"

// ---- PixelUnshuffle(P) of an NCHW map as rows [B h w, ld] ------------------------------------------------------------------------------
// One work item = one DESTINATION element: consecutive lanes write consecutive columns of a row and read runs of P consecutive
// source pixels.  Columns [C P P, ld) are the K padding of the GEMM that follows: zeros.
template <typename TI, typename TO>
__global__ __launch_bounds__(256) void unshuffle_rows_kernel(const typename TI::storage* __restrict__ src, typename TO::storage* __restrict__ dst,
                                                             int C, int h, int w, int P, int64_t ld, int64_t n) {
    const int PP = P * P, CPP = C * PP;
    const int64_t Hd = (int64_t)h * P, Wd = (int64_t)w * P;
    for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < n; it += (int64_t)gridDim.x * 256) {
        const int col = (int)(it % ld);
        float val = 0.f;
        if (col < CPP) {
            const int64_t tok = it / ld;
            const int c = col / PP, u = (col - c * PP) / P, v = col - c * PP - u * P;
            const int64_t j = tok % w, i = (tok / w) % h, b = tok / ((int64_t)w * h);
            val = TI::load(src + ((b * C + c) * Hd + i * P + u) * Wd + j * P + v);
        }
        TO::store(dst + it, val);
    }
}

// the adjoint: one work item = one element of the NCHW map (a permutation: every real column is read once, the pad columns never)
template <typename TI>
__global__ __launch_bounds__(256) void unshuffle_rows_bwd_kernel(const typename TI::storage* __restrict__ rows, float* __restrict__ dst,
                                                                 int C, int h, int w, int P, int64_t ld, int64_t n) {
    const int PP = P * P;
    const int64_t Hd = (int64_t)h * P, Wd = (int64_t)w * P;
    for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < n; it += (int64_t)gridDim.x * 256) {
        const int64_t x = it % Wd, y = (it / Wd) % Hd, bc = it / (Wd * Hd);
        const int c = (int)(bc % C);
        const int64_t b = bc / C, i = y / P, j = x / P;
        const int u = (int)(y - i * P), v = (int)(x - j * P);
        dst[it] = TI::load(rows + ((b * h + i) * w + j) * ld + c * PP + u * P + v);
    }
}

// ---- y = act(x) ------------------------------------------------------------------------------------------------------------------------
// exact-erf GELU (libm erff, as the fp32 GEMM's epilogue and uc_act_bwd) or ReLU, evaluated in fp32.  Each work item reads its
// elements before it writes them, so y may be x.
__device__ __forceinline__ float act_apply(float x, int act) {
    return act == UC_ACT_GELU_ERF ? 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)) : fmaxf(x, 0.f);
}

template <typename Tag, bool VEC>
__global__ __launch_bounds__(256) void act_kernel(const typename Tag::storage* x, typename Tag::storage* y, int act, int64_t n) {
    const int64_t n4 = VEC ? n / 4 : 0;
    for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < n4; it += (int64_t)gridDim.x * 256) {
        float4_t v = vec_load4<Tag>(x + it * 4);
        v.x = act_apply(v.x, act); v.y = act_apply(v.y, act); v.z = act_apply(v.z, act); v.w = act_apply(v.w, act);
        vec_store4<Tag>(y + it * 4, v);
    }
    // the tail of the vector form (n % 4 elements), or everything when a pointer is not aligned for 4-element accesses
    for (int64_t i = n4 * 4 + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        Tag::store(y + i, act_apply(Tag::load(x + i), act));
}

// ---- y = LN2(LN1(x) + pe) --------------------------------------------------------------------------------------------------------------
// One wavefront per row, 4 rows per workgroup, the row in registers (C <= 64 * 4 * LPL_MAXV), like uc_layernorm's kernels
// (rope_norm.hip): two-pass statistics, per-lane partial sums over the lane's chunks in ascending order, then the wave butterfly.
// Each of the three steps is skipped when its pointer is NULL (a wave-uniform branch).  A single norm without pe and without mid IS
// uc_layernorm and is handed to it by the entry point (the same statements compile to other FMA contractions in another kernel, so
// only the same kernel gives the same bits).
#define LPL_MAXV 8

struct LplArgs {
    const float *g1, *b1, *pe, *g2, *b2;
    float* mid;
    float eps1, eps2;
    int64_t rows, N;
    int C;
};

// v <- (v - mean) rstd gamma + beta over the lane's chunks; EX: every chunk is inside the row
template <int NI, bool EX>
__device__ __forceinline__ void lpl_norm(float4_t (&v)[NI], int C, int lane, const float* __restrict__ gamma, const float* __restrict__ beta,
                                         float eps) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NI; ++i)
        if (EX || (i * 64 + lane) * 4 < C) s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    const float mean = wave_sum(s) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NI; ++i)
        if (EX || (i * 64 + lane) * 4 < C) {
            const float a = v[i].x - mean, b = v[i].y - mean, d = v[i].z - mean, e = v[i].w - mean;
            q += (a * a + b * b) + (d * d + e * e);
        }
    const float rstd = rsqrtf(wave_sum(q) / (float)C + eps);
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int c = (i * 64 + lane) * 4;
        if (EX || c < C) {
            const float4_t g = *reinterpret_cast<const float4_t*>(gamma + c);
            const float4_t bb = *reinterpret_cast<const float4_t*>(beta + c);
            v[i].x = (v[i].x - mean) * rstd * g.x + bb.x;
            v[i].y = (v[i].y - mean) * rstd * g.y + bb.y;
            v[i].z = (v[i].z - mean) * rstd * g.z + bb.z;
            v[i].w = (v[i].w - mean) * rstd * g.w + bb.w;
        }
    }
}

// NI chunks of 256 channels per row.  EX: C == NI * 256, no per-chunk predicates, all loads of a row issued back to back; else any
// C % 4 == 0 up to NI * 256 (the compiler hoists every gamma / beta / pe load of the row: the register count grows with NI, so a
// narrow row takes a narrow instantiation)
template <typename TI, typename TO, int NI, bool EX>
__global__ __launch_bounds__(256) void ln_pe_ln_vec_kernel(const typename TI::storage* __restrict__ x, typename TO::storage* __restrict__ y, LplArgs a) {
    const int C = EX ? NI * 256 : a.C;
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.rows) return;
    const typename TI::storage* xr = x + row * C;
    float4_t v[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int c = (i * 64 + lane) * 4;
        if (EX || c < C) v[i] = vec_load4<TI>(xr + c);
    }
    if (a.g1) lpl_norm<NI, EX>(v, C, lane, a.g1, a.b1, a.eps1);
    if (a.pe) {
        const float* per = a.pe + (row % a.N) * C;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int c = (i * 64 + lane) * 4;
            if (EX || c < C) v[i] += *reinterpret_cast<const float4_t*>(per + c);
        }
    }
    if (a.mid) {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int c = (i * 64 + lane) * 4;
            if (EX || c < C) *reinterpret_cast<float4_t*>(a.mid + row * C + c) = v[i];
        }
    }
    if (a.g2) lpl_norm<NI, EX>(v, C, lane, a.g2, a.b2, a.eps2);
    typename TO::storage* yr = y + row * C;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int c = (i * 64 + lane) * 4;
        if (EX || c < C) vec_store4<TO>(yr + c, v[i]);
    }
}

// any C, any alignment: scalar accesses, the (cache-resident) row re-read per pass, the LN2 input re-evaluated instead of stored
template <typename TI, typename TO>
__global__ __launch_bounds__(256) void ln_pe_ln_scalar_kernel(const typename TI::storage* __restrict__ x, typename TO::storage* __restrict__ y, LplArgs a) {
    const int C = a.C;
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.rows) return;
    const typename TI::storage* xr = x + row * C;
    const float* per = a.pe ? a.pe + (row % a.N) * C : nullptr;
    float mean1 = 0.f, rstd1 = 1.f;
    if (a.g1) {
        float s = 0.f;
        for (int c = lane; c < C; c += 64) s += TI::load(xr + c);
        mean1 = wave_sum(s) / (float)C;
        float q = 0.f;
        for (int c = lane; c < C; c += 64) {
            const float d = TI::load(xr + c) - mean1;
            q += d * d;
        }
        rstd1 = rsqrtf(wave_sum(q) / (float)C + a.eps1);
    }
    auto mid_at = [&](int c) {
        float t = TI::load(xr + c);
        if (a.g1) t = (t - mean1) * rstd1 * a.g1[c] + a.b1[c];
        if (per) t += per[c];
        return t;
    };
    float mean2 = 0.f, rstd2 = 1.f;
    if (a.g2) {
        float s = 0.f;
        for (int c = lane; c < C; c += 64) s += mid_at(c);
        mean2 = wave_sum(s) / (float)C;
        float q = 0.f;
        for (int c = lane; c < C; c += 64) {
            const float d = mid_at(c) - mean2;
            q += d * d;
        }
        rstd2 = rsqrtf(wave_sum(q) / (float)C + a.eps2);
    }
    for (int c = lane; c < C; c += 64) {
        float t = mid_at(c);
        if (a.mid) a.mid[row * C + c] = t;
        if (a.g2) t = (t - mean2) * rstd2 * a.g2[c] + a.b2[c];
        TO::store(y + row * C + c, t);
    }
}

// ---- entry points ----------------------------------------------------------------------------------------------------------------------
static int unshuffle_check(const char* fn, const void* a, const void* b, int B, int C, int h, int w, int P, int64_t ld) {
    UC_REQUIRE(a && b, "%s: null pointer", fn);
    UC_REQUIRE(B > 0 && C > 0 && h > 0 && w > 0 && P > 0, "%s: bad shape B=%d C=%d h=%d w=%d P=%d", fn, B, C, h, w, P);
    UC_REQUIRE((int64_t)C * P * P <= 0x7fffffff && (int64_t)h * P <= 0x7fffffff && (int64_t)w * P <= 0x7fffffff,
               "%s: C P P, h P and w P must stay below 2^31 (C=%d h=%d w=%d P=%d)", fn, C, h, w, P);
    UC_REQUIRE(ld >= (int64_t)C * P * P && ld <= 0x7fffffff, "%s: ld=%lld is smaller than C P P = %lld (or beyond 2^31)", fn, (long long)ld,
               (long long)C * P * P);
    return UC_OK;
}

template <typename TI>
static int unshuffle_launch(const char* fn, const void* src, void* dst, int dst_dtype, int C, int h, int w, int P, int64_t ld, int64_t n, hipStream_t st) {
    UC_DISPATCH(fn, dst_dtype, hipLaunchKernelGGL((unshuffle_rows_kernel<TI, Tag>), dim3(EW_GRID(n)), dim3(256), 0, st, (const typename TI::storage*)src, (Tag::storage*)dst, C, h, w, P, ld, n));
    return UC_OK;
}

extern "C" int uc_unshuffle_rows(const void* src, int src_dtype, void* dst, int dst_dtype, int B, int C, int h, int w, int P, int64_t ld,
                                 uc_stream_t stream) {
    const char* fn = "uc_unshuffle_rows";
    UC_REQUIRE_DTYPE(fn, src_dtype, false);
    UC_REQUIRE_DTYPE(fn, dst_dtype, false);
    if (int e = unshuffle_check(fn, src, dst, B, C, h, w, P, ld)) return e;
    const int64_t n = (int64_t)B * h * w * ld;
    hipStream_t st = (hipStream_t)stream;
    if (int e = src_dtype == UC_F32 ? unshuffle_launch<F32Tag>(fn, src, dst, dst_dtype, C, h, w, P, ld, n, st)
                                    : unshuffle_launch<BF16Tag>(fn, src, dst, dst_dtype, C, h, w, P, ld, n, st)) return e;
    UC_CHECK_LAUNCH(fn);
    return UC_OK;
}

extern "C" int uc_unshuffle_rows_bwd(const void* rows, int rows_dtype, float* dst, int B, int C, int h, int w, int P, int64_t ld,
                                     uc_stream_t stream) {
    const char* fn = "uc_unshuffle_rows_bwd";
    UC_REQUIRE_DTYPE(fn, rows_dtype, false);
    if (int e = unshuffle_check(fn, rows, dst, B, C, h, w, P, ld)) return e;
    const int64_t n = (int64_t)B * C * h * P * w * P;
    UC_DISPATCH(fn, rows_dtype, hipLaunchKernelGGL((unshuffle_rows_bwd_kernel<Tag>), dim3(EW_GRID(n)), dim3(256), 0, (hipStream_t)stream, (const Tag::storage*)rows, dst, C, h, w, P, ld, n));
    UC_CHECK_LAUNCH(fn);
    return UC_OK;
}

extern "C" int uc_act(const void* x, void* y, int dtype, int act, int64_t n, uc_stream_t stream) {
    const char* fn = "uc_act";
    UC_REQUIRE_DTYPE(fn, dtype, false);
    UC_REQUIRE(x && y && n >= 0, "%s: bad argument (null pointer or n=%lld)", fn, (long long)n);
    UC_REQUIRE(act == UC_ACT_GELU_ERF || act == UC_ACT_RELU, "%s: bad act %d (UC_ACT_GELU_ERF or UC_ACT_RELU)", fn, act);
    if (n == 0) return UC_OK;
    hipStream_t st = (hipStream_t)stream;
    const uintptr_t align = dtype == UC_F32 ? 16 : 8;          // four elements
    if ((uintptr_t)x % align == 0 && (uintptr_t)y % align == 0)
        UC_DISPATCH(fn, dtype, hipLaunchKernelGGL((act_kernel<Tag, true>), dim3(EW_GRID(ceil_div64(n, 4))), dim3(256), 0, st, (const Tag::storage*)x, (Tag::storage*)y, act, n));
    else
        UC_DISPATCH(fn, dtype, hipLaunchKernelGGL((act_kernel<Tag, false>), dim3(EW_GRID(n)), dim3(256), 0, st, (const Tag::storage*)x, (Tag::storage*)y, act, n));
    UC_CHECK_LAUNCH(fn);
    return UC_OK;
}

template <typename TI, typename TO>
static void lpl_launch(const void* x, void* y, const LplArgs& a, bool vec, hipStream_t st) {
    typedef typename TI::storage SI;
    typedef typename TO::storage SO;
    const dim3 grid((unsigned)ceil_div64(a.rows, 4));
#define LPL_VEC(NI_, EX_) hipLaunchKernelGGL((ln_pe_ln_vec_kernel<TI, TO, NI_, EX_>), grid, dim3(256), 0, st, (const SI*)x, (SO*)y, a)
    if (vec && a.C == 1024) LPL_VEC(4, true);
    else if (vec && a.C == 768) LPL_VEC(3, true);
    else if (vec && a.C == 1536) LPL_VEC(6, true);
    else if (vec && a.C == 2048) LPL_VEC(8, true);
    else if (vec && a.C <= 256) LPL_VEC(1, false);
    else if (vec && a.C <= 512) LPL_VEC(2, false);
    else if (vec && a.C <= 1024) LPL_VEC(4, false);
    else if (vec) LPL_VEC(LPL_MAXV, false);
#undef LPL_VEC
    else hipLaunchKernelGGL((ln_pe_ln_scalar_kernel<TI, TO>), grid, dim3(256), 0, st, (const SI*)x, (SO*)y, a);
}

template <typename TI>
static int lpl_dispatch_out(const char* fn, const void* x, void* y, int y_dtype, const LplArgs& a, bool vec, hipStream_t st) {
    UC_DISPATCH(fn, y_dtype, (lpl_launch<TI, Tag>(x, y, a, vec, st)));
    return UC_OK;
}

extern "C" int uc_ln_pe_ln(const void* x, int x_dtype, const float* gamma1, const float* beta1, float eps1, const float* pe, const float* gamma2,
                           const float* beta2, float eps2, void* y, int y_dtype, float* mid, int64_t B, int64_t N, int C, uc_stream_t stream) {
    const char* fn = "uc_ln_pe_ln";
    UC_REQUIRE_DTYPE(fn, x_dtype, false);
    UC_REQUIRE_DTYPE(fn, y_dtype, false);
    UC_REQUIRE(x && y, "%s: null pointer", fn);
    UC_REQUIRE(B > 0 && N > 0 && C > 0 && B <= 0x7fffffff && N <= 0x7fffffff && (B * N + 3) / 4 <= 0x7fffffff, "%s: bad shape B=%lld N=%lld C=%d", fn,
               (long long)B, (long long)N, C);
    UC_REQUIRE((gamma1 != nullptr) == (beta1 != nullptr) && (gamma2 != nullptr) == (beta2 != nullptr),
               "%s: a norm takes gamma and beta together (both NULL: Identity)", fn);
    UC_REQUIRE(gamma1 || pe || gamma2, "%s: nothing to do (LN1, pe and LN2 are all NULL)", fn);
    UC_REQUIRE((!gamma1 || eps1 > 0.f) && (!gamma2 || eps2 > 0.f), "%s: eps must be positive (eps1=%g eps2=%g)", fn, (double)eps1, (double)eps2);
    if (!pe && !mid && !(gamma1 && gamma2))      // one norm and nothing else: uc_layernorm itself, bit for bit
        return uc_layernorm(x, x_dtype, gamma1 ? gamma1 : gamma2, gamma1 ? beta1 : beta2, y, y_dtype, B * N, C, gamma1 ? eps1 : eps2, stream);
    LplArgs a;
    a.g1 = gamma1; a.b1 = beta1; a.pe = pe; a.g2 = gamma2; a.b2 = beta2; a.mid = mid;
    a.eps1 = eps1; a.eps2 = eps2; a.rows = B * N; a.N = N; a.C = C;
    const bool f32_16 = ((uintptr_t)gamma1 | (uintptr_t)beta1 | (uintptr_t)pe | (uintptr_t)gamma2 | (uintptr_t)beta2 | (uintptr_t)mid) % 16 == 0;
    const bool vec = C % 4 == 0 && C <= 64 * 4 * LPL_MAXV && f32_16 && (uintptr_t)x % 16 == 0 && (uintptr_t)y % 16 == 0;
    hipStream_t st = (hipStream_t)stream;
    if (int e = x_dtype == UC_F32 ? lpl_dispatch_out<F32Tag>(fn, x, y, y_dtype, a, vec, st) : lpl_dispatch_out<BF16Tag>(fn, x, y, y_dtype, a, vec, st)) return e;
    UC_CHECK_LAUNCH(fn);
    return UC_OK;
}

// ---- dgamma, dbeta of y = LN(x) in a fixed order ---------------------------------------------------------------------------------------
// uc_layernorm_bwd adds its dgamma / dbeta partial sums with fp32 atomics: their last bits change from run to run.  Here every sum has
// one order: (1) one wavefront per row forms (mean, rstd) (two-pass, as the forward); (2) one thread per column adds up
// dy x^ and dy over the LPG_ROWS rows of its slab, rows ascending; (3) one thread per column adds up the slabs, ascending.  The
// workspace (caller-provided) holds the row statistics and the slab partials.
#define LPG_ROWS 64

template <typename TX>
__global__ __launch_bounds__(256) void ln_row_stats_kernel(const typename TX::storage* __restrict__ x, float2* __restrict__ stats, int64_t rows, int C,
                                                           float eps) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const typename TX::storage* xr = x + row * C;
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += TX::load(xr + c);
    const float mean = wave_sum(s) / (float)C;
    float q = 0.f;
    for (int c = lane; c < C; c += 64) {
        const float d = TX::load(xr + c) - mean;
        q += d * d;
    }
    const float rstd = rsqrtf(wave_sum(q) / (float)C + eps);
    if (lane == 0) stats[row] = make_float2(mean, rstd);
}

// partial [slabs][2][C]: slab blockIdx.y, column blockIdx.x * 256 + threadIdx.x (consecutive lanes on consecutive columns of a row)
template <typename TX, typename TD>
__global__ __launch_bounds__(256) void ln_param_grads_slab_kernel(const typename TX::storage* __restrict__ x, const typename TD::storage* __restrict__ dy,
                                                                  const float2* __restrict__ stats, float* __restrict__ partial, int64_t rows, int C) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const int64_t r0 = (int64_t)blockIdx.y * LPG_ROWS, r1 = min(rows, r0 + LPG_ROWS);
    float dg = 0.f, db = 0.f;
    for (int64_t r = r0; r < r1; ++r) {
        const float2 st = stats[r];
        const float g = TD::load(dy + r * C + c);
        dg += g * ((TX::load(x + r * C + c) - st.x) * st.y);
        db += g;
    }
    partial[((int64_t)blockIdx.y * 2 + 0) * C + c] = dg;
    partial[((int64_t)blockIdx.y * 2 + 1) * C + c] = db;
}

__global__ __launch_bounds__(256) void ln_param_grads_merge_kernel(const float* __restrict__ partial, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                                   int64_t slabs, int C) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    float dg = 0.f, db = 0.f;
    for (int64_t s = 0; s < slabs; ++s) {
        dg += partial[(s * 2 + 0) * C + c];
        db += partial[(s * 2 + 1) * C + c];
    }
    dgamma[c] = dg;
    dbeta[c] = db;
}

extern "C" int64_t uc_ln_param_grads_ws_bytes(int64_t rows, int64_t C) {
    if (rows <= 0 || C <= 0) return 0;
    return (int64_t)sizeof(float) * (2 * rows + 2 * C * ceil_div64(rows, LPG_ROWS));
}

template <typename TX>
static int lpg_launch(const char* fn, const void* x, const void* dy, int dy_dtype, float2* stats, float* partial, int64_t rows, int C, float eps,
                      int64_t slabs, hipStream_t st) {
    hipLaunchKernelGGL((ln_row_stats_kernel<TX>), dim3((unsigned)ceil_div64(rows, 4)), dim3(256), 0, st, (const typename TX::storage*)x, stats, rows, C, eps);
    const dim3 grid((unsigned)ceil_div64(C, 256), (unsigned)slabs);
    UC_DISPATCH(fn, dy_dtype, hipLaunchKernelGGL((ln_param_grads_slab_kernel<TX, Tag>), grid, dim3(256), 0, st, (const typename TX::storage*)x, (const Tag::storage*)dy, stats, partial, rows, C));
    return UC_OK;
}

extern "C" int uc_ln_param_grads(const void* x, int x_dtype, const void* dy, int dy_dtype, float* dgamma, float* dbeta, float* ws, int64_t rows, int C,
                                 float eps, uc_stream_t stream) {
    const char* fn = "uc_ln_param_grads";
    UC_REQUIRE_DTYPE(fn, x_dtype, false);
    UC_REQUIRE_DTYPE(fn, dy_dtype, false);
    UC_REQUIRE(x && dy && dgamma && dbeta && ws, "%s: null pointer", fn);
    UC_REQUIRE(rows > 0 && C > 0 && (rows + 3) / 4 <= 0x7fffffff && ceil_div64(rows, LPG_ROWS) <= 65535, "%s: bad shape rows=%lld C=%d (at most %d rows)", fn,
               (long long)rows, C, 65535 * LPG_ROWS);
    UC_REQUIRE(eps > 0.f, "%s: eps must be positive (eps=%g)", fn, (double)eps);
    UC_REQUIRE((uintptr_t)ws % 8 == 0, "%s: ws must be 8-byte aligned", fn);
    const int64_t slabs = ceil_div64(rows, LPG_ROWS);
    float2* stats = (float2*)ws;
    float* partial = ws + 2 * rows;
    hipStream_t st = (hipStream_t)stream;
    if (int e = x_dtype == UC_F32 ? lpg_launch<F32Tag>(fn, x, dy, dy_dtype, stats, partial, rows, C, eps, slabs, st)
                                  : lpg_launch<BF16Tag>(fn, x, dy, dy_dtype, stats, partial, rows, C, eps, slabs, st)) return e;
    hipLaunchKernelGGL(ln_param_grads_merge_kernel, dim3((unsigned)ceil_div64(C, 256)), dim3(256), 0, st, partial, dgamma, dbeta, slabs, C);
    UC_CHECK_LAUNCH(fn);
    return UC_OK;
}
