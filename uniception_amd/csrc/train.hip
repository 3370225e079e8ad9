// Backward / training-step kernels of the DUSt3R path that are HBM-bound: LayerNorm backward, column sums (bias
// gradients), activation backward, 2-D transpose (puts the reduction axis of the weight-gradient GEMMs on the
// contiguous dimension), fused adaptor+loss forward/backward, pixel un-shuffle, AdamW.
// The reference has no hand-written backward (it is PyTorch autograd over the modules); each kernel cites the forward
// expression it differentiates in include/uc_hip.h.
#include "vec_access.h"
#include "layernorm_plan.h"
#include <algorithm>

// ---------------------------------------------------------------------------------------------------------------
// LayerNorm backward.  One wavefront per row, exact width C = NV*256 (all loads of a row issued back to back), rows
// distributed grid-stride so each wave also accumulates its share of dgamma/dbeta in registers and issues ONE atomic
// per column at the end.
// ---------------------------------------------------------------------------------------------------------------
// a lane's four values as they lie in memory (kept packed while in flight)
template <typename T> struct TrRaw;
template <> struct TrRaw<F32Tag> {
    typedef float4_t type;
    static __device__ __forceinline__ float4_t unpack(float4_t r) { return r; }
};
template <> struct TrRaw<BF16Tag> {
    typedef uint2 type;
    static __device__ __forceinline__ float4_t unpack(uint2 r) { return unpack_bf16x4(r); }
};

__device__ __forceinline__ void wave_sum2(float& a, float& b) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o, 64);
        b += __shfl_xor(b, o, 64);
    }
}

// TX: dtype of the residual stream (x, dres, dx): fp32, or bf16 — the bf16 training stream of round 4 (the reference's stream under
// autocast: bf16 activations, bf16 gradients of them): 2 + 2 + 2 + 2 bytes per element instead of 4 + 2 + 4 + 4 + 2.
template <typename TD, int NV, typename TX = F32Tag>
__global__ __launch_bounds__(512) void layernorm_bwd_kernel(const typename TX::storage* __restrict__ x, const float* __restrict__ gamma,
                                                            const typename TD::storage* __restrict__ dy,
                                                            const typename TX::storage* __restrict__ dres, typename TX::storage* __restrict__ dx,
                                                            bf16_t* __restrict__ dx_b, float* __restrict__ dgamma,
                                                            float* __restrict__ dbeta, int64_t rows, float eps) {
    constexpr int C = NV * 256;
    __shared__ float red[2 * C];   // block-level dgamma | dbeta (LDS atomics), then ONE global atomic per column per block
    const int lane = threadIdx.x & 63;
    const int64_t wave_id = (int64_t)blockIdx.x * 8 + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * 8;
    for (int i = threadIdx.x; i < 2 * C; i += 512) red[i] = 0.f;
    float4_t g[NV], dg[NV], db[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        g[i] = *reinterpret_cast<const float4_t*>(gamma + (i * 64 + lane) * 4);
        dg[i] = (float4_t){0.f, 0.f, 0.f, 0.f};
        db[i] = (float4_t){0.f, 0.f, 0.f, 0.f};
    }
    const float invC = 1.0f / (float)C;
    // One row per wave and iteration; the NEXT row's operands are requested (raw: 8 bytes per lane and vector for bf16) before this row's
    // arithmetic starts — with one row in flight per wave (2048 waves x 6 KB) the kernel ran at 3.5 TB/s.
    typedef typename TrRaw<TX>::type rawx_t;
    typedef typename TrRaw<TD>::type rawd_t;
    rawx_t nx[NV], nr[NV];
    rawd_t nd[NV];
    auto request = [&](int64_t row) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < NV; ++i) nx[i] = *reinterpret_cast<const rawx_t*>(x + row * C + (i * 64 + lane) * 4);
#pragma unroll
        for (int i = 0; i < NV; ++i) nd[i] = *reinterpret_cast<const rawd_t*>(dy + row * C + (i * 64 + lane) * 4);
        if (dres) {
#pragma unroll
            for (int i = 0; i < NV; ++i) nr[i] = *reinterpret_cast<const rawx_t*>(dres + row * C + (i * 64 + lane) * 4);
        }
    };
    if (wave_id < rows) request(wave_id);
    for (int64_t row = wave_id; row < rows; row += nwaves) {
        float4_t v[NV], d[NV], rs[NV];
#pragma unroll
        for (int i = 0; i < NV; ++i) { v[i] = TrRaw<TX>::unpack(nx[i]); d[i] = TrRaw<TD>::unpack(nd[i]); }
        if (dres) {
#pragma unroll
            for (int i = 0; i < NV; ++i) rs[i] = TrRaw<TX>::unpack(nr[i]);
        }
        if (row + nwaves < rows) request(row + nwaves);
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
        const float mean = wave_sum(s) * invC;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            v[i].x -= mean; v[i].y -= mean; v[i].z -= mean; v[i].w -= mean;
            q += (v[i].x * v[i].x + v[i].y * v[i].y) + (v[i].z * v[i].z + v[i].w * v[i].w);
        }
        const float rstd = rsqrtf(wave_sum(q) * invC + eps);
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            v[i].x *= rstd; v[i].y *= rstd; v[i].z *= rstd; v[i].w *= rstd;   // xhat
            dg[i].x += d[i].x * v[i].x; dg[i].y += d[i].y * v[i].y; dg[i].z += d[i].z * v[i].z; dg[i].w += d[i].w * v[i].w;
            db[i].x += d[i].x; db[i].y += d[i].y; db[i].z += d[i].z; db[i].w += d[i].w;
            d[i].x *= g[i].x; d[i].y *= g[i].y; d[i].z *= g[i].z; d[i].w *= g[i].w;               // a = dy*gamma
            s1 += (d[i].x + d[i].y) + (d[i].z + d[i].w);
            s2 += (d[i].x * v[i].x + d[i].y * v[i].y) + (d[i].z * v[i].z + d[i].w * v[i].w);
        }
        wave_sum2(s1, s2);
        s1 *= invC; s2 *= invC;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            float4_t o;
            o.x = rstd * (d[i].x - s1 - v[i].x * s2);
            o.y = rstd * (d[i].y - s1 - v[i].y * s2);
            o.z = rstd * (d[i].z - s1 - v[i].z * s2);
            o.w = rstd * (d[i].w - s1 - v[i].w * s2);
            if (dres) { o.x += rs[i].x; o.y += rs[i].y; o.z += rs[i].z; o.w += rs[i].w; }
            vec_store4<TX>(dx + row * C + (i * 64 + lane) * 4, o);
            if (dx_b) {   // bf16 twin of dx: the operand the previous sub-layer's backward GEMMs will want
                uint2 pk;
                pk.x = pack_bf16x2(o.x, o.y);
                pk.y = pack_bf16x2(o.z, o.w);
                *reinterpret_cast<uint2*>(dx_b + row * C + (i * 64 + lane) * 4) = pk;
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = (i * 64 + lane) * 4;
        atomicAdd(red + c + 0, dg[i].x); atomicAdd(red + c + 1, dg[i].y);
        atomicAdd(red + c + 2, dg[i].z); atomicAdd(red + c + 3, dg[i].w);
        atomicAdd(red + C + c + 0, db[i].x); atomicAdd(red + C + c + 1, db[i].y);
        atomicAdd(red + C + c + 2, db[i].z); atomicAdd(red + C + c + 3, db[i].w);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < C; i += 512) {
        unsafeAtomicAdd(dgamma + i, red[i]);
        unsafeAtomicAdd(dbeta + i, red[C + i]);
    }
}

// C = 64 (round 5): LayerNorm over head_dim — qk_norm, utils/transformer_blocks.py:196-197 — has B N H rows of 64: 16 lanes x 4 channels
// per row, four rows per wave and iteration (512 contiguous bytes per bf16 load), row sums over 16 lanes, dgamma / dbeta kept per lane
// over the wave's rows and added once per block (the any-width kernel below would issue one atomic per ELEMENT on 64 addresses).
__device__ __forceinline__ float row16_sum(float v) {
    v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 4, 64); v += __shfl_xor(v, 8, 64);
    return v;
}
template <typename TD, typename TX>
__global__ __launch_bounds__(256) void layernorm64_bwd_kernel(const typename TX::storage* __restrict__ x, const float* __restrict__ gamma,
                                                              const typename TD::storage* __restrict__ dy, typename TX::storage* __restrict__ dx,
                                                              float* __restrict__ dgamma, float* __restrict__ dbeta, int64_t rows, float eps) {
    __shared__ float red[128];
    const int lane = threadIdx.x & 63, sub = lane & 15, rg = lane >> 4;
    const int64_t wave_id = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
    if (threadIdx.x < 128) red[threadIdx.x] = 0.f;
    const float4_t g = *reinterpret_cast<const float4_t*>(gamma + 4 * sub);
    float4_t dg = {0.f, 0.f, 0.f, 0.f}, db = {0.f, 0.f, 0.f, 0.f};
    for (int64_t r0 = wave_id * 4; r0 < rows; r0 += nwaves * 4) {
        const int64_t row = r0 + rg;
        const bool ok = row < rows;
        float4_t v = {0.f, 0.f, 0.f, 0.f}, d = {0.f, 0.f, 0.f, 0.f};
        if (ok) { v = vec_load4<TX>(x + row * 64 + 4 * sub); d = vec_load4<TD>(dy + row * 64 + 4 * sub); }
        const float mean = row16_sum((v.x + v.y) + (v.z + v.w)) * (1.0f / 64.0f);
        v.x -= mean; v.y -= mean; v.z -= mean; v.w -= mean;
        const float rstd = rsqrtf(row16_sum((v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w)) * (1.0f / 64.0f) + eps);
        v.x *= rstd; v.y *= rstd; v.z *= rstd; v.w *= rstd;                                     // xhat
        dg.x += d.x * v.x; dg.y += d.y * v.y; dg.z += d.z * v.z; dg.w += d.w * v.w;
        db.x += d.x; db.y += d.y; db.z += d.z; db.w += d.w;
        d.x *= g.x; d.y *= g.y; d.z *= g.z; d.w *= g.w;                                         // a = dy * gamma
        const float s1 = row16_sum((d.x + d.y) + (d.z + d.w)) * (1.0f / 64.0f);
        const float s2 = row16_sum((d.x * v.x + d.y * v.y) + (d.z * v.z + d.w * v.w)) * (1.0f / 64.0f);
        if (ok) {
            float4_t o;
            o.x = rstd * (d.x - s1 - v.x * s2); o.y = rstd * (d.y - s1 - v.y * s2);
            o.z = rstd * (d.z - s1 - v.z * s2); o.w = rstd * (d.w - s1 - v.w * s2);
            vec_store4<TX>(dx + row * 64 + 4 * sub, o);
        }
    }
#pragma unroll
    for (int o = 16; o < 64; o <<= 1) {      // the wave's four row groups
        dg.x += __shfl_xor(dg.x, o, 64); dg.y += __shfl_xor(dg.y, o, 64); dg.z += __shfl_xor(dg.z, o, 64); dg.w += __shfl_xor(dg.w, o, 64);
        db.x += __shfl_xor(db.x, o, 64); db.y += __shfl_xor(db.y, o, 64); db.z += __shfl_xor(db.z, o, 64); db.w += __shfl_xor(db.w, o, 64);
    }
    __syncthreads();
    if (rg == 0) {
        atomicAdd(red + 4 * sub + 0, dg.x); atomicAdd(red + 4 * sub + 1, dg.y); atomicAdd(red + 4 * sub + 2, dg.z); atomicAdd(red + 4 * sub + 3, dg.w);
        atomicAdd(red + 64 + 4 * sub + 0, db.x); atomicAdd(red + 64 + 4 * sub + 1, db.y); atomicAdd(red + 64 + 4 * sub + 2, db.z); atomicAdd(red + 64 + 4 * sub + 3, db.w);
    }
    __syncthreads();
    if (threadIdx.x < 64) {
        unsafeAtomicAdd(dgamma + threadIdx.x, red[threadIdx.x]);
        unsafeAtomicAdd(dbeta + threadIdx.x, red[64 + threadIdx.x]);
    }
}

// any width: one wavefront per row, three strided passes, per-element atomics for dgamma/dbeta (small models only)
template <typename TD, typename TX = F32Tag>
__global__ __launch_bounds__(256) void layernorm_bwd_generic_kernel(const typename TX::storage* __restrict__ x, const float* __restrict__ gamma,
                                                                    const typename TD::storage* __restrict__ dy,
                                                                    const typename TX::storage* __restrict__ dres, typename TX::storage* __restrict__ dx,
                                                                    bf16_t* __restrict__ dx_b, float* __restrict__ dgamma,
                                                                    float* __restrict__ dbeta, int64_t rows, int C, float eps) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const typename TX::storage* xr = x + row * C;
    const typename TD::storage* dr = dy + row * C;
    const float invC = 1.0f / (float)C;
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += TX::load(xr + c);
    const float mean = wave_sum(s) * invC;
    float q = 0.f;
    for (int c = lane; c < C; c += 64) { const float d = TX::load(xr + c) - mean; q += d * d; }
    const float rstd = rsqrtf(wave_sum(q) * invC + eps);
    float s1 = 0.f, s2 = 0.f;
    for (int c = lane; c < C; c += 64) {
        const float xh = (TX::load(xr + c) - mean) * rstd, a = TD::load(dr + c) * gamma[c];
        s1 += a; s2 += a * xh;
    }
    wave_sum2(s1, s2);
    s1 *= invC; s2 *= invC;
    for (int c = lane; c < C; c += 64) {
        const float xh = (TX::load(xr + c) - mean) * rstd, d = TD::load(dr + c);
        float o = rstd * (d * gamma[c] - s1 - xh * s2);
        if (dres) o += TX::load(dres + row * C + c);
        TX::store(dx + row * C + c, o);
        if (dx_b) dx_b[row * C + c] = f32_to_bf16(o);
        unsafeAtomicAdd(dgamma + c, d * xh);
        unsafeAtomicAdd(dbeta + c, d);
    }
}

extern "C" int uc_layernorm_bwd(const void* x, int x_dtype, const float* gamma, const void* dy, int dy_dtype, const void* dres, void* dx,
                                void* dx_bf16, float* dgamma, float* dbeta, int64_t rows, int C, float eps, uc_stream_t stream) {
    bf16_t* dx_b = (bf16_t*)dx_bf16;
    UC_REQUIRE(x && gamma && dy && dx && dgamma && dbeta, "uc_layernorm_bwd: null pointer");
    UC_REQUIRE(rows >= 0 && C > 0, "uc_layernorm_bwd: bad shape");
    UC_REQUIRE(dy_dtype == UC_F32 || dy_dtype == UC_BF16, "uc_layernorm_bwd: bad dy dtype %d", dy_dtype);
    UC_REQUIRE(x_dtype == UC_F32 || x_dtype == UC_BF16, "uc_layernorm_bwd: bad x dtype %d", x_dtype);
    UC_REQUIRE(x_dtype == UC_F32 || !dx_bf16, "uc_layernorm_bwd: a bf16 stream's dx is its own bf16 copy (dx_bf16 must be NULL)");
    if (rows == 0) return UC_OK;
    hipStream_t st = (hipStream_t)stream;
    const bool xb = x_dtype == UC_BF16;
    const LnBwdPlan p = uc_ln_bwd_plan(rows, C, dres != nullptr, dx_bf16 != nullptr, xb ? 2 : 4, dy_dtype == UC_BF16 ? 2 : 4, (uintptr_t)x,
                                       (uintptr_t)dy, (uintptr_t)dres, (uintptr_t)dx, (uintptr_t)dx_bf16, (uintptr_t)gamma);
    if (p.kernel == UC_LN_BWD_C64) {
        const unsigned g64 = p.grid;
#define UC_LN64(TD_, TX_)                                                                                                               \
        hipLaunchKernelGGL((layernorm64_bwd_kernel<TD_, TX_>), dim3(g64), dim3(256), 0, st, (const typename TX_::storage*)x, gamma,        \
                           (const typename TD_::storage*)dy, (typename TX_::storage*)dx, dgamma, dbeta, rows, eps)
        if (dy_dtype == UC_F32) { if (xb) UC_LN64(F32Tag, BF16Tag); else UC_LN64(F32Tag, F32Tag); }
        else { if (xb) UC_LN64(BF16Tag, BF16Tag); else UC_LN64(BF16Tag, F32Tag); }
#undef UC_LN64
        UC_CHECK_LAUNCH("uc_layernorm_bwd");
        return UC_OK;
    }
    if (p.kernel == UC_LN_BWD_GENERIC) {
        const unsigned g = p.grid;
#define UC_LNG(TD_, TX_)                                                                                                                \
        hipLaunchKernelGGL((layernorm_bwd_generic_kernel<TD_, TX_>), dim3(g), dim3(256), 0, st, (const typename TX_::storage*)x, gamma,     \
                           (const typename TD_::storage*)dy, (const typename TX_::storage*)dres, (typename TX_::storage*)dx, dx_b, dgamma, dbeta, rows, C, eps)
        if (dy_dtype == UC_F32) { if (xb) UC_LNG(F32Tag, BF16Tag); else UC_LNG(F32Tag, F32Tag); }
        else { if (xb) UC_LNG(BF16Tag, BF16Tag); else UC_LNG(BF16Tag, F32Tag); }
#undef UC_LNG
        UC_CHECK_LAUNCH("uc_layernorm_bwd");
        return UC_OK;
    }
    const unsigned grid = p.grid;
#define UC_LNB(TD_, NV_, TX_)                                                                                                       \
    hipLaunchKernelGGL((layernorm_bwd_kernel<TD_, NV_, TX_>), dim3(grid), dim3(512), 0, st, (const typename TX_::storage*)x, gamma,      \
                       (const typename TD_::storage*)dy, (const typename TX_::storage*)dres, (typename TX_::storage*)dx, dx_b, dgamma, dbeta, rows, eps)
#define UC_LNB_NV(TD_, TX_)                      \
    switch (p.nv) {                              \
        case 1: UC_LNB(TD_, 1, TX_); break;      \
        case 2: UC_LNB(TD_, 2, TX_); break;      \
        case 3: UC_LNB(TD_, 3, TX_); break;      \
        case 4: UC_LNB(TD_, 4, TX_); break;      \
        case 6: UC_LNB(TD_, 6, TX_); break;      \
        case 8: UC_LNB(TD_, 8, TX_); break;      \
        default: uc_set_error("uc_layernorm_bwd: unsupported width %d", C); return UC_ERR_UNSUPPORTED; \
    }
    if (dy_dtype == UC_F32) { if (xb) { UC_LNB_NV(F32Tag, BF16Tag) } else { UC_LNB_NV(F32Tag, F32Tag) } }
    else { if (xb) { UC_LNB_NV(BF16Tag, BF16Tag) } else { UC_LNB_NV(BF16Tag, F32Tag) } }
#undef UC_LNB_NV
#undef UC_LNB
    UC_CHECK_LAUNCH("uc_layernorm_bwd");
    return UC_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// column sums: block = 64 column-lanes (4 columns each) x 4 row-lanes; grid.y slabs of rows; one atomic per column per block
// ---------------------------------------------------------------------------------------------------------------
template <typename Tag>
__global__ __launch_bounds__(256) void colsum_kernel(const typename Tag::storage* __restrict__ src, int64_t M, int64_t N,
                                                     int64_t ld, float* __restrict__ out, int64_t rows_per_block) {
    __shared__ float red[4][64][4];
    const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int64_t c0 = ((int64_t)blockIdx.x * 64 + cl) * 4;
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_block;
    const int64_t r1 = min(M, r0 + rows_per_block);
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    if (c0 + 3 < N && (ld % 4 == 0)) {
        int64_t r = r0 + rl;
        for (; r + 12 < r1; r += 16) {   // 4 independent loads in flight
            const float4_t v0 = vec_load4<Tag>(src + r * ld + c0), v1 = vec_load4<Tag>(src + (r + 4) * ld + c0);
            const float4_t v2 = vec_load4<Tag>(src + (r + 8) * ld + c0), v3 = vec_load4<Tag>(src + (r + 12) * ld + c0);
            a[0] += (v0.x + v1.x) + (v2.x + v3.x); a[1] += (v0.y + v1.y) + (v2.y + v3.y);
            a[2] += (v0.z + v1.z) + (v2.z + v3.z); a[3] += (v0.w + v1.w) + (v2.w + v3.w);
        }
        for (; r < r1; r += 4) {
            const float4_t v = vec_load4<Tag>(src + r * ld + c0);
            a[0] += v.x; a[1] += v.y; a[2] += v.z; a[3] += v.w;
        }
    } else {
        for (int64_t r = r0 + rl; r < r1; r += 4)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (c0 + e < N) a[e] += Tag::load(src + r * ld + c0 + e);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) red[rl][cl][e] = a[e];
    __syncthreads();
    if (rl == 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float s = red[0][cl][e] + red[1][cl][e] + red[2][cl][e] + red[3][cl][e];
            if (c0 + e < N) unsafeAtomicAdd(out + c0 + e, s);
        }
    }
}

extern "C" int uc_colsum(const void* src, int dtype, int64_t M, int64_t N, int64_t ld, float* out, uc_stream_t stream) {
    UC_REQUIRE(src && out && M >= 0 && N > 0 && ld >= N, "uc_colsum: bad argument");
    if (M == 0) return UC_OK;
    // row slabs: enough blocks to fill the chip (~2048 in total), never so many that the per-block column atomics
    // (fp32 atomics sustain only ~75 G/s) outweigh the streaming: 8.4 M rows x 128 columns with 64-row slabs = 8.4 M atomics
    const unsigned gx = (unsigned)ceil_div64(N, 256);
    const int64_t max_slabs = max((int64_t)1, (int64_t)2048 / gx);
    dim3 grid(gx, (unsigned)min(max_slabs, ceil_div64(M, 64)));
    const int64_t rpb = ceil_div64(M, grid.y);
    hipStream_t st = (hipStream_t)stream;
    UC_DISPATCH("uc_colsum", dtype, hipLaunchKernelGGL((colsum_kernel<Tag>), grid, dim3(256), 0, st, (const Tag::storage*)src, M, N, ld, out, rpb));
    UC_CHECK_LAUNCH("uc_colsum");
    return UC_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// split-K reduction: out[i] (+)= sum_s ws[s*slab_stride + i]   (the slabs written by uc_gemm / uc_gemm_tn)
// ---------------------------------------------------------------------------------------------------------------
__global__ void splitk_reduce_kernel(const float* __restrict__ ws, int sk, int64_t n4, int64_t stride4, float* __restrict__ out, int accumulate) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        float4_t a = accumulate ? reinterpret_cast<const float4_t*>(out)[i] : (float4_t){0.f, 0.f, 0.f, 0.f};
        for (int s = 0; s < sk; ++s) {
            const float4_t v = reinterpret_cast<const float4_t*>(ws)[(int64_t)s * stride4 + i];
            a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
        }
        reinterpret_cast<float4_t*>(out)[i] = a;
    }
}

extern "C" int uc_splitk_reduce(const float* ws, int split_k, int64_t n, int64_t slab_stride, float* out, int accumulate,
                                uc_stream_t stream) {
    UC_REQUIRE(ws && out && split_k >= 1 && n > 0 && n % 4 == 0 && slab_stride >= n && slab_stride % 4 == 0,
               "uc_splitk_reduce: bad argument (n and slab_stride must be multiples of 4)");
    UC_REQUIRE(((uintptr_t)ws % 16 == 0) && ((uintptr_t)out % 16 == 0), "uc_splitk_reduce: ws and out must be 16-byte aligned (float4 accesses)");
    const int64_t n4 = n / 4;
    const unsigned grid = (unsigned)min((int64_t)8192, ceil_div64(n4, 256));
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, ws, split_k, n4, slab_stride / 4, out, accumulate);
    UC_CHECK_LAUNCH("uc_splitk_reduce");
    return UC_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// activation backward
// ---------------------------------------------------------------------------------------------------------------
template <typename Tag>
__global__ void act_bwd_kernel(const typename Tag::storage* __restrict__ dg, const typename Tag::storage* __restrict__ u,
                               typename Tag::storage* __restrict__ du, int act, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float x = Tag::load(u + i), g = Tag::load(dg + i);
        float d;
        if (act == UC_ACT_GELU_ERF) {
            // d/dx [0.5 x (1 + erf(x/sqrt2))] = 0.5 (1 + erf(x/sqrt2)) + x exp(-x^2/2) / sqrt(2 pi)
            d = 0.5f * (1.0f + erff(x * 0.70710678118654752440f)) + x * expf(-0.5f * x * x) * 0.39894228040143267794f;
        } else {
            d = x > 0.f ? 1.f : 0.f;
        }
        Tag::store(du + i, g * d);
    }
}

extern "C" int uc_act_bwd(const void* dg, const void* u, void* du, int dtype, int act, int64_t n, uc_stream_t stream) {
    UC_REQUIRE(dg && u && du && n >= 0, "uc_act_bwd: bad argument");
    UC_REQUIRE(act == UC_ACT_GELU_ERF || act == UC_ACT_RELU, "uc_act_bwd: bad act %d", act);
    if (n == 0) return UC_OK;
    hipStream_t st = (hipStream_t)stream;
    UC_DISPATCH("uc_act_bwd", dtype,
                hipLaunchKernelGGL((act_bwd_kernel<Tag>), dim3(EW_GRID(n)), dim3(256), 0, st, (const Tag::storage*)dg, (const Tag::storage*)u, (Tag::storage*)du, act, n));
    UC_CHECK_LAUNCH("uc_act_bwd");
    return UC_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Dropout / DropPath in training (round 5; nn.Dropout on a sub-layer's output or hidden activation, timm's DropPath on the sub-layer's
// branch — blocks.py:64-86, 120-161; transformer_blocks.py:145-208): out = (residual +) x * (mask ? scale : 0).  mask: one byte per
// element (rows_per_mask == 0) or one byte per group of rows_per_mask consecutive rows (DropPath: one per sample).  The same kernel is
// the backward (on the gradient, without residual).  HBM-bound; four elements per lane (cols % 4 == 0).
// ---------------------------------------------------------------------------------------------------------------
template <typename TX, typename TO>
__global__ __launch_bounds__(256) void mask_scale_kernel(const typename TX::storage* __restrict__ x, const unsigned char* __restrict__ mask,
                                                         const typename TO::storage* __restrict__ residual, typename TO::storage* __restrict__ out,
                                                         int64_t n4, int cols4, int64_t rows_per_mask, float scale) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        float4_t v = vec_load4<TX>(x + i * 4);
        float4_t m;
        if (rows_per_mask > 0) {
            const float k = mask[(i / cols4) / rows_per_mask] ? scale : 0.f;
            m = (float4_t){k, k, k, k};
        } else {
            const unsigned w = *reinterpret_cast<const unsigned*>(mask + i * 4);
            m = (float4_t){(w & 0xffu) ? scale : 0.f, (w & 0xff00u) ? scale : 0.f, (w & 0xff0000u) ? scale : 0.f, (w & 0xff000000u) ? scale : 0.f};
        }
        v.x *= m.x; v.y *= m.y; v.z *= m.z; v.w *= m.w;
        if (residual) {
            const float4_t r = vec_load4<TO>(residual + i * 4);
            v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w;
        }
        vec_store4<TO>(out + i * 4, v);
    }
}

extern "C" int uc_mask_scale(const void* x, int x_dtype, const unsigned char* mask, int64_t rows_per_mask, float scale, const void* residual,
                             void* out, int out_dtype, int64_t rows, int cols, uc_stream_t stream) {
    UC_REQUIRE(x && mask && out && rows >= 0 && cols > 0 && cols % 4 == 0 && rows_per_mask >= 0, "uc_mask_scale: bad argument");
    UC_REQUIRE((x_dtype == UC_F32 || x_dtype == UC_BF16) && (out_dtype == UC_F32 || out_dtype == UC_BF16), "uc_mask_scale: fp32 / bf16 tensors only");
    if (rows == 0) return UC_OK;
    const int64_t n4 = rows * (cols / 4);
    const unsigned grid = (unsigned)min((int64_t)65536, ceil_div64(n4, 256));
    hipStream_t st = (hipStream_t)stream;
#define UC_MS(TX_, TO_)                                                                                                                   \
    hipLaunchKernelGGL((mask_scale_kernel<TX_, TO_>), dim3(grid), dim3(256), 0, st, (const typename TX_::storage*)x, mask,                    \
                       (const typename TO_::storage*)residual, (typename TO_::storage*)out, n4, cols / 4, rows_per_mask, scale)
    if (x_dtype == UC_F32) { if (out_dtype == UC_F32) UC_MS(F32Tag, F32Tag); else UC_MS(F32Tag, BF16Tag); }
    else { if (out_dtype == UC_F32) UC_MS(BF16Tag, F32Tag); else UC_MS(BF16Tag, BF16Tag); }
#undef UC_MS
    UC_CHECK_LAUNCH("uc_mask_scale");
    return UC_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// SwiGLU gate of DINOv2's giant FFN (the hub's SwiGLUFFNFused: x1, x2 = w12(x).chunk(2); w3(silu(x1) * x2)):
//   forward   g[m, j] = silu(t[m, j]) * t[m, H + j]                                        t [M, 2H] -> g [M, H]
//   backward  dt[m, j] = dg x2 s (1 + x1 (1 - s)),  dt[m, H + j] = dg x1 s,  s = sigmoid(x1)
// HBM-bound (3 / 5 values per gate element): one lane per 8 consecutive columns, 16-byte loads and stores for the 16-bit dtypes
// (H % 8 == 0; launcher), grid-stride over M * H / 8 items.
// ---------------------------------------------------------------------------------------------------------------
template <typename Tag, bool BWD>
__global__ __launch_bounds__(256) void swiglu_kernel(const typename Tag::storage* __restrict__ t, const typename Tag::storage* __restrict__ dg,
                                                     typename Tag::storage* __restrict__ out, int64_t M, int H, uc_fastdiv dPer) {
    typedef typename Tag::storage S;
    const unsigned per_row = (unsigned)H / 8u;
    const int64_t items = M * per_row;
    for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += (int64_t)gridDim.x * blockDim.x) {
        // (items of one launch chunk stay below 2^31: launcher)
        const unsigned m = uc_div((unsigned)it, dPer), j = ((unsigned)it - m * per_row) * 8u;
        const S* row = t + (int64_t)m * 2 * H;
        S a[8], b[8], g[8];
        __builtin_memcpy(a, row + j, sizeof(a));
        __builtin_memcpy(b, row + H + j, sizeof(b));
        if (BWD) __builtin_memcpy(g, dg + (int64_t)m * H + j, sizeof(g));
        S o1[8], o2[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const float x1 = Tag::load(a + r), x2 = Tag::load(b + r);
            const float s = 1.0f / (1.0f + __expf(-x1));
            if (BWD) {
                const float d = Tag::load(g + r);
                Tag::store(o1 + r, d * x2 * s * (1.0f + x1 * (1.0f - s)));
                Tag::store(o2 + r, d * x1 * s);
            } else {
                Tag::store(o1 + r, x1 * s * x2);
            }
        }
        if (BWD) {
            S* orow = out + (int64_t)m * 2 * H;
            __builtin_memcpy(orow + j, o1, sizeof(o1));
            __builtin_memcpy(orow + H + j, o2, sizeof(o2));
        } else {
            __builtin_memcpy(out + (int64_t)m * H + j, o1, sizeof(o1));
        }
    }
}

template <bool BWD>
static int swiglu_launch(const void* t, const void* dg, void* out, int dtype, int64_t M, int64_t H, hipStream_t st, const char* who) {
    if (M == 0) return UC_OK;
    const uc_fastdiv d = uc_make_fastdiv((unsigned)(H / 8));
    const int64_t rows_per = std::max<int64_t>(1, (((int64_t)1 << 31) - 1) / (H / 8));          // 32-bit item index per launch
    for (int64_t m0 = 0; m0 < M; m0 += rows_per) {
        const int64_t mc = std::min(rows_per, M - m0);
        const unsigned grid = (unsigned)std::min<int64_t>((int64_t)uc_num_cus() * 16, ceil_div64(mc * (H / 8), 256));
        UC_DISPATCH(who, dtype,
                    hipLaunchKernelGGL((swiglu_kernel<Tag, BWD>), dim3(grid), dim3(256), 0, st, (const Tag::storage*)t + m0 * 2 * H,
                                       dg ? (const Tag::storage*)dg + m0 * H : nullptr, (Tag::storage*)out + m0 * (BWD ? 2 : 1) * H, mc, (int)H, d));
    }
    return UC_OK;
}

extern "C" int uc_swiglu(const void* t, void* g, int dtype, int64_t M, int64_t H, uc_stream_t stream) {
    UC_REQUIRE(t && g && M >= 0 && H > 0 && H % 8 == 0 && H < ((int64_t)1 << 28), "uc_swiglu: bad argument (H must be a positive multiple of 8)");
    if (int rc = swiglu_launch<false>(t, nullptr, g, dtype, M, H, (hipStream_t)stream, "uc_swiglu")) return rc;
    UC_CHECK_LAUNCH("uc_swiglu");
    return UC_OK;
}

extern "C" int uc_swiglu_bwd(const void* dg, const void* t, void* dt, int dtype, int64_t M, int64_t H, uc_stream_t stream) {
    UC_REQUIRE(dg && t && dt && M >= 0 && H > 0 && H % 8 == 0 && H < ((int64_t)1 << 28), "uc_swiglu_bwd: bad argument (H must be a positive multiple of 8)");
    if (int rc = swiglu_launch<true>(t, dg, dt, dtype, M, H, (hipStream_t)stream, "uc_swiglu_bwd")) return rc;
    UC_CHECK_LAUNCH("uc_swiglu_bwd");
    return UC_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// 2-D transpose, 64x64 tiles through LDS (pitch 65 floats: conflict-free both ways)
// ---------------------------------------------------------------------------------------------------------------
template <typename TI, typename TO>
__global__ __launch_bounds__(256) void transpose64_kernel(const typename TI::storage* __restrict__ src,
                                                          typename TO::storage* __restrict__ dst,
                                                          typename TO::storage* __restrict__ copy, int64_t R, int64_t S,
                                                          int64_t ld_dst, int rows_on_x) {
    __shared__ float tile[64][65];
    // (the longer tile axis rides on grid.x, whose limit is 2^31 - 1: a [4 M pixels, C] gradient map has 65 536 row tiles — one more
    //  than grid.y takes; round 6: the fp32-class heads' training step at bench sizes)
    const int64_t s0 = (int64_t)(rows_on_x ? blockIdx.y : blockIdx.x) * 64, r0 = (int64_t)(rows_on_x ? blockIdx.x : blockIdx.y) * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int64_t r = r0 + ty + 4 * k, s = s0 + tx;
        float v = 0.f;
        if (r < R && s < S) {
            v = TI::load(src + r * S + s);
            if (copy) TO::store(copy + r * S + s, v);
        }
        tile[ty + 4 * k][tx] = v;   // rows >= R read back as the zero padding of dst
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int64_t s = s0 + ty + 4 * k, r = r0 + tx;
        if (r < ld_dst && s < S) TO::store(dst + s * ld_dst + r, tile[tx][ty + 4 * k]);
    }
}

extern "C" int uc_transpose2d(const void* src, int sd, void* dst, int dd, void* rowmajor_copy, int64_t R, int64_t S,
                              int64_t ld_dst, uc_stream_t stream) {
    UC_REQUIRE(src && dst && R > 0 && S > 0, "uc_transpose2d: bad argument");
    UC_REQUIRE(ld_dst >= R && ld_dst < R + 64, "uc_transpose2d: ld_dst must be in [R, R+64)");
    const int64_t tiles_s = ceil_div64(S, 64), tiles_r = ceil_div64(ld_dst, 64);
    const int rows_on_x = tiles_r > tiles_s;
    UC_REQUIRE(std::min(tiles_s, tiles_r) <= 65535 && std::max(tiles_s, tiles_r) < ((int64_t)1 << 31), "uc_transpose2d: matrix exceeds the launch grid");
    dim3 grid((unsigned)(rows_on_x ? tiles_r : tiles_s), (unsigned)(rows_on_x ? tiles_s : tiles_r));
    hipStream_t st = (hipStream_t)stream;
    if (sd == UC_BF16 && dd == UC_BF16) hipLaunchKernelGGL((transpose64_kernel<BF16Tag, BF16Tag>), grid, dim3(256), 0, st, (const bf16_t*)src, (bf16_t*)dst, (bf16_t*)rowmajor_copy, R, S, ld_dst, rows_on_x);
    else if (sd == UC_F32 && dd == UC_F32) hipLaunchKernelGGL((transpose64_kernel<F32Tag, F32Tag>), grid, dim3(256), 0, st, (const float*)src, (float*)dst, (float*)rowmajor_copy, R, S, ld_dst, rows_on_x);
    else if (sd == UC_F32 && dd == UC_BF16) hipLaunchKernelGGL((transpose64_kernel<F32Tag, BF16Tag>), grid, dim3(256), 0, st, (const float*)src, (bf16_t*)dst, (bf16_t*)rowmajor_copy, R, S, ld_dst, rows_on_x);
    else if (sd == UC_F16 && dd == UC_F16) hipLaunchKernelGGL((transpose64_kernel<F16Tag, F16Tag>), grid, dim3(256), 0, st, (const unsigned short*)src, (unsigned short*)dst, (unsigned short*)rowmajor_copy, R, S, ld_dst, rows_on_x);
    else { uc_set_error("uc_transpose2d: unsupported dtypes %d -> %d", sd, dd); return UC_ERR_BAD_ARG; }
    UC_CHECK_LAUNCH("uc_transpose2d");
    return UC_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// fused adaptor + confidence-weighted regression loss, forward and backward
//   pts = xyz * s(d), s(d) = expm1(d)/max(d,1e-8), d = |xyz|;  conf = 1 + exp(c)
//   L = conf * r - alpha * log(conf),  r = |pts - gt|
//   dL/dpts = conf * (pts-gt)/max(r,1e-12);  dL/dc = (r - alpha/conf) * exp(c)
//   dpts_i/dxyz_j = s delta_ij + xyz_i xyz_j s'(d)/d,  s'(d) = (exp(d) d - expm1(d)) / d^2
// ---------------------------------------------------------------------------------------------------------------
__global__ void pointmap_loss_kernel(const float* __restrict__ x, int64_t sb, int64_t sc, int64_t sp,
                                     const float* __restrict__ gt, float alpha, float gscale, float* __restrict__ loss_sum,
                                     float* __restrict__ dx, int64_t HW, int64_t n) {
    float local = 0.f;
    for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < n; it += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = it / HW, pix = it % HW;
        const int64_t base = b * sb + pix * sp;
        const float X = x[base], Y = x[base + sc], Z = x[base + 2 * sc], Cf = x[base + 3 * sc];
        const float d = sqrtf(X * X + Y * Y + Z * Z);
        const float dc = fmaxf(d, 1e-8f);
        const float em1 = expm1f(d);
        const float s = em1 / dc;
        const float px = X * s, py = Y * s, pz = Z * s;
        const float ec = expf(Cf);
        const float conf = 1.0f + ec;
        const float ex = px - gt[it * 3 + 0], ey = py - gt[it * 3 + 1], ez = pz - gt[it * 3 + 2];
        const float r = sqrtf(ex * ex + ey * ey + ez * ez);
        local += conf * r - alpha * logf(conf);
        const float ir = conf / fmaxf(r, 1e-12f);
        const float gx = ex * ir, gy = ey * ir, gz = ez * ir;          // dL/dpts
        // s'(d) = (e^d d - expm1(d)) / d^2, series 1/2 + d/3 near 0 (the closed form cancels catastrophically there)
        const float sprime = (d > 1e-2f) ? ((em1 + 1.0f) * d - em1) / (d * d) : 0.5f + d * (1.0f / 3.0f);
        const float sprime_over_d = sprime / dc;
        const float dot = X * gx + Y * gy + Z * gz;
        const float k = dot * sprime_over_d;
        dx[base] = (s * gx + X * k) * gscale;
        dx[base + sc] = (s * gy + Y * k) * gscale;
        dx[base + 2 * sc] = (s * gz + Z * k) * gscale;
        dx[base + 3 * sc] = (r - alpha / conf) * ec * gscale;
    }
    local = wave_sum(local);
    if ((threadIdx.x & 63) == 0) unsafeAtomicAdd(loss_sum, local);
}

extern "C" int uc_pointmap_loss(const float* x, int64_t x_sb, int64_t x_sc, int64_t x_sp, const float* gt, float alpha,
                                float grad_scale, float* loss_sum, float* dx, int B, int H, int W, uc_stream_t stream) {
    UC_REQUIRE(x && gt && loss_sum && dx && B > 0 && H > 0 && W > 0, "uc_pointmap_loss: bad argument");
    const int64_t n = (int64_t)B * H * W;
    const unsigned grid = (unsigned)min((int64_t)4096, ceil_div64(n, 256));
    hipLaunchKernelGGL(pointmap_loss_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, x_sb, x_sc, x_sp, gt, alpha,
                       grad_scale, loss_sum, dx, (int64_t)H * W, n);
    UC_CHECK_LAUNCH("uc_pointmap_loss");
    return UC_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// adaptor backward alone (arbitrary downstream loss): dx from (dpts, dconf)
// ---------------------------------------------------------------------------------------------------------------
__global__ void pointmap_adaptor_bwd_kernel(const float* __restrict__ x, int64_t sb, int64_t sc, int64_t sp,
                                            const float* __restrict__ dpts, const float* __restrict__ dconf, float cspan,
                                            float* __restrict__ dx, int64_t HW, int64_t n) {
    for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < n; it += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = it / HW, pix = it % HW;
        const int64_t base = b * sb + pix * sp;
        const float X = x[base], Y = x[base + sc], Z = x[base + 2 * sc], Cf = x[base + 3 * sc];
        const float d = sqrtf(X * X + Y * Y + Z * Z);
        const float dc = fmaxf(d, 1e-8f);
        const float em1 = expm1f(d);
        const float s = em1 / dc;
        const float sprime = (d > 1e-2f) ? ((em1 + 1.0f) * d - em1) / (d * d) : 0.5f + d * (1.0f / 3.0f);
        const float gx = dpts ? dpts[it * 3 + 0] : 0.f, gy = dpts ? dpts[it * 3 + 1] : 0.f, gz = dpts ? dpts[it * 3 + 2] : 0.f;
        const float k = (X * gx + Y * gy + Z * gz) * sprime / dc;
        dx[base] = s * gx + X * k;
        dx[base + sc] = s * gy + Y * k;
        dx[base + 2 * sc] = s * gz + Z * k;
        const float ec = expf(Cf);
        // conf = vmin + min(exp(c), vmax - vmin): gradient passes only below the clamp
        dx[base + 3 * sc] = (dconf && ec < cspan) ? dconf[it] * ec : 0.f;
    }
}

extern "C" int uc_pointmap_adaptor_bwd(const float* x, int64_t x_sb, int64_t x_sc, int64_t x_sp, const float* dpts,
                                       const float* dconf, float conf_vmin, float conf_vmax, float* dx, int B, int H, int W,
                                       uc_stream_t stream) {
    UC_REQUIRE(x && dx && B > 0 && H > 0 && W > 0, "uc_pointmap_adaptor_bwd: bad argument");
    const int64_t n = (int64_t)B * H * W;
    const unsigned grid = (unsigned)min((int64_t)8192, ceil_div64(n, 256));
    hipLaunchKernelGGL(pointmap_adaptor_bwd_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, x_sb, x_sc, x_sp, dpts,
                       dconf, conf_vmax - conf_vmin, dx, (int64_t)H * W, n);
    UC_CHECK_LAUNCH("uc_pointmap_adaptor_bwd");
    return UC_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// confidence-weighted regression loss on adaptor outputs: sum_pix conf*|pts-gt| - alpha*log(conf), with both gradients
// ---------------------------------------------------------------------------------------------------------------
__global__ void conf_loss_kernel(const float* __restrict__ pts, const float* __restrict__ conf, const float* __restrict__ gt,
                                 float alpha, float gscale, float* __restrict__ loss_sum, float* __restrict__ dpts,
                                 float* __restrict__ dconf, int64_t n) {
    float local = 0.f;
    for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < n; it += (int64_t)gridDim.x * blockDim.x) {
        const float ex = pts[it * 3 + 0] - gt[it * 3 + 0], ey = pts[it * 3 + 1] - gt[it * 3 + 1], ez = pts[it * 3 + 2] - gt[it * 3 + 2];
        const float r = sqrtf(ex * ex + ey * ey + ez * ez);
        const float c = conf[it];
        local += c * r - alpha * logf(c);
        const float ir = gscale * c / fmaxf(r, 1e-12f);
        dpts[it * 3 + 0] = ex * ir; dpts[it * 3 + 1] = ey * ir; dpts[it * 3 + 2] = ez * ir;
        dconf[it] = gscale * (r - alpha / c);
    }
    local = wave_sum(local);
    if ((threadIdx.x & 63) == 0) unsafeAtomicAdd(loss_sum, local);
}

extern "C" int uc_conf_loss(const float* pts, const float* conf, const float* gt, float alpha, float grad_scale,
                            float* loss_sum, float* dpts, float* dconf, int64_t npix, uc_stream_t stream) {
    UC_REQUIRE(pts && conf && gt && loss_sum && dpts && dconf && npix > 0, "uc_conf_loss: bad argument");
    const unsigned grid = (unsigned)min((int64_t)8192, ceil_div64(npix, 256));
    hipLaunchKernelGGL(conf_loss_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, pts, conf, gt, alpha, grad_scale,
                       loss_sum, dpts, dconf, npix);
    UC_CHECK_LAUNCH("uc_conf_loss");
    return UC_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// pixel un-shuffle (gradient of the linear head's pixel_shuffle)
// ---------------------------------------------------------------------------------------------------------------
template <typename TO>
__global__ void pixel_unshuffle_kernel(const float* __restrict__ src, typename TO::storage* __restrict__ dst, int B, int h, int w,
                                       int P, int Cout, int64_t n) {
    const int Wd = P * w, Hd = P * h, CPP = Cout * P * P;
    for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < n; it += (int64_t)gridDim.x * blockDim.x) {
        // destination order: (token row, column c*P*P + u*P + v)
        const int col = (int)(it % CPP);
        const int64_t tok = it / CPP;
        const int v = col % P, u = (col / P) % P, c = col / (P * P);
        const int j = (int)(tok % w), i = (int)((tok / w) % h), b = (int)(tok / ((int64_t)w * h));
        TO::store(dst + it, src[(((int64_t)b * Cout + c) * Hd + (int64_t)i * P + u) * Wd + (int64_t)j * P + v]);
    }
}

extern "C" int uc_pixel_unshuffle(const float* src, void* dst, int dst_dtype, int B, int h, int w, int P, int Cout, uc_stream_t stream) {
    UC_REQUIRE(src && dst && B > 0 && h > 0 && w > 0 && P > 0 && Cout > 0, "uc_pixel_unshuffle: bad argument");
    const int64_t n = (int64_t)B * h * w * Cout * P * P;
    hipStream_t st = (hipStream_t)stream;
    UC_DISPATCH("uc_pixel_unshuffle", dst_dtype,
                hipLaunchKernelGGL((pixel_unshuffle_kernel<Tag>), dim3(EW_GRID(n)), dim3(256), 0, st, src, (Tag::storage*)dst, B, h, w, P, Cout, n));
    UC_CHECK_LAUNCH("uc_pixel_unshuffle");
    return UC_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// AdamW on flat fp32 buffers (decoupled weight decay, bias-corrected moments)
// ---------------------------------------------------------------------------------------------------------------
__global__ void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                             int64_t n, float lr, float b1, float b2, float eps, float wd, float c1, float c2, float gs) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float gi = g[i] * gs;
        const float mi = b1 * m[i] + (1.f - b1) * gi;
        const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
        m[i] = mi;
        v[i] = vi;
        const float upd = (mi * c1) / (sqrtf(vi * c2) + eps);
        p[i] = p[i] * (1.f - lr * wd) - lr * upd;
    }
}

extern "C" int uc_adamw(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                        float weight_decay, int step, float grad_scale, uc_stream_t stream) {
    UC_REQUIRE(p && g && m && v && n >= 0 && step >= 1, "uc_adamw: bad argument");
    if (n == 0) return UC_OK;
    const float c1 = 1.0f / (1.0f - powf(beta1, (float)step));
    const float c2 = 1.0f / (1.0f - powf(beta2, (float)step));
    const unsigned grid = (unsigned)min((int64_t)65536, ceil_div64(n, 256));
    hipLaunchKernelGGL(adamw_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, lr, beta1, beta2, eps,
                       weight_decay, c1, c2, grad_scale);
    UC_CHECK_LAUNCH("uc_adamw");
    return UC_OK;
}
