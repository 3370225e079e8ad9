// Token pooling of the summary heads (PoseHead / GlobalHead: AdaptiveAvgPool2d(1) over the token matrix) and its adjoint.
//
// Both kernels stream: every element is read or written once, 16 bytes per lane, a wave covering 1 KiB of one row.
//   forward : B x C outputs alone are a handful of workgroups, so T is cut into chunks of POOL_CHUNK rows; a workgroup sums one chunk
//             of 64 column groups (its four waves take rows t0 + w, t0 + w + 4, ... in ascending order, the four wave sums are added
//             in wave order) and stores the partial; a second kernel adds the partials in chunk order and divides by T.  No float
//             atomics: the same bits on every run.
//   backward: out[b T + t, c] = g[b, c] / T, times (gate[b T + t, c] > 0) when a gate is given (the ReLU of the last res_conv3 under
//             the residual sum) — the broadcast map is never stored on its own.
#include "vec_access.h"

#define POOL_CHUNK 64   // rows of T per workgroup of the first stage
#define POOL_WAVES 4

template <typename Tag>
struct PoolVec {
    static constexpr int V = 16 / (int)sizeof(typename Tag::storage);   // elements of one 16-byte access
    union Pack {
        uint4 q;
        typename Tag::storage e[16 / sizeof(typename Tag::storage)];
    };
};

// v[0..V) = the V elements at p (one 16-byte load), or the first nvalid of them element by element (the last column group of a
// row whose C is no multiple of V: nothing past column C is touched)
template <typename Tag>
__device__ __forceinline__ void pool_load(const typename Tag::storage* __restrict__ p, int nvalid, float (&v)[PoolVec<Tag>::V]) {
    constexpr int V = PoolVec<Tag>::V;
    if (nvalid >= V) {
        typename PoolVec<Tag>::Pack pk;
        pk.q = *reinterpret_cast<const uint4*>(p);
#pragma unroll
        for (int k = 0; k < V; ++k) v[k] = Tag::load(&pk.e[k]);
    } else {
#pragma unroll
        for (int k = 0; k < V; ++k) v[k] = k < nvalid ? Tag::load(p + k) : 0.f;
    }
}

template <typename Tag>
__device__ __forceinline__ void pool_store(typename Tag::storage* __restrict__ p, int nvalid, const float (&v)[PoolVec<Tag>::V]) {
    constexpr int V = PoolVec<Tag>::V;
    if (nvalid >= V) {
        typename PoolVec<Tag>::Pack pk;
#pragma unroll
        for (int k = 0; k < V; ++k) Tag::store(&pk.e[k], v[k]);
        *reinterpret_cast<uint4*>(p) = pk.q;
    } else {
#pragma unroll
        for (int k = 0; k < V; ++k)
            if (k < nvalid) Tag::store(p + k, v[k]);
    }
}

// grid (column-group blocks, chunks of T, B); partial [B][nchunk][C] fp32
template <typename Tag>
__global__ __launch_bounds__(64 * POOL_WAVES) void token_pool_partial_kernel(const typename Tag::storage* __restrict__ x, int64_t ld,
                                                                            float* __restrict__ partial, int T, int C, int nchunk) {
    constexpr int V = PoolVec<Tag>::V;
    __shared__ float red[POOL_WAVES][64][V];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t c0 = ((int64_t)blockIdx.x * 64 + lane) * V;
    const int chunk = blockIdx.y;
    const int64_t b = blockIdx.z;
    const int t0 = chunk * POOL_CHUNK, t1 = min(T, t0 + POOL_CHUNK);
    const int nvalid = c0 < C ? (int)min((int64_t)V, (int64_t)C - c0) : 0;
    float acc[V];
#pragma unroll
    for (int k = 0; k < V; ++k) acc[k] = 0.f;
    if (nvalid > 0) {
        const typename Tag::storage* base = x + b * T * ld + c0;
#pragma unroll 4
        for (int t = t0 + wave; t < t1; t += POOL_WAVES) {
            float v[V];
            pool_load<Tag>(base + (int64_t)t * ld, nvalid, v);
#pragma unroll
            for (int k = 0; k < V; ++k) acc[k] += v[k];
        }
    }
#pragma unroll
    for (int k = 0; k < V; ++k) red[wave][lane][k] = acc[k];
    __syncthreads();
    if (wave == 0 && nvalid > 0) {
        float* dst = partial + (b * nchunk + chunk) * (int64_t)C + c0;
#pragma unroll
        for (int k = 0; k < V; ++k)
            if (k < nvalid) dst[k] = ((red[0][lane][k] + red[1][lane][k]) + red[2][lane][k]) + red[3][lane][k];
    }
}

// one thread per output: the chunk partials of (b, c) added in chunk order
__global__ __launch_bounds__(256) void token_pool_reduce_kernel(const float* __restrict__ partial, float* __restrict__ out, int64_t total,
                                                                int T, int C, int nchunk) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int64_t b = i / C;
    const int64_t c = i - b * C;
    const float* p = partial + b * nchunk * (int64_t)C + c;
    float s = 0.f;
    for (int k = 0; k < nchunk; ++k) s += p[(int64_t)k * C];
    out[i] = s / (float)T;
}

// one thread per (row, column group)
template <typename Tag>
__global__ __launch_bounds__(256) void token_pool_bwd_kernel(const float* __restrict__ g, const typename Tag::storage* __restrict__ gate,
                                                             int64_t ld_gate, typename Tag::storage* __restrict__ out, int64_t ld_out,
                                                             int64_t total, int T, int C, int ngroups) {
    constexpr int V = PoolVec<Tag>::V;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int64_t row = i / ngroups;
    const int c0 = (int)(i - row * ngroups) * V;
    const int nvalid = min(V, C - c0);
    const float* gb = g + (row / T) * C + c0;
    float v[V];
#pragma unroll
    for (int k = 0; k < V; ++k) v[k] = k < nvalid ? gb[k] / (float)T : 0.f;
    if (gate) {
        float u[V];
        pool_load<Tag>(gate + row * ld_gate + c0, nvalid, u);
#pragma unroll
        for (int k = 0; k < V; ++k) v[k] = u[k] > 0.f ? v[k] : 0.f;
    }
    pool_store<Tag>(out + row * ld_out + c0, nvalid, v);
}

static inline int64_t pool_chunks(int64_t T) { return (T + POOL_CHUNK - 1) / POOL_CHUNK; }
static inline int pool_vec(int dtype) { return dtype == UC_F32 ? 4 : 8; }

extern "C" int64_t uc_token_pool_ws_bytes(int64_t B, int64_t T, int64_t C) {
    if (B <= 0 || T <= 0 || C <= 0) return 0;
    return B * pool_chunks(T) * C * (int64_t)sizeof(float);
}

extern "C" int uc_token_pool(const void* x, int dtype, int64_t ld, float* out, float* ws, int64_t B, int64_t T, int64_t C,
                             uc_stream_t stream) {
    const char* fn = "uc_token_pool";
    UC_REQUIRE(x && out && ws, "%s: null pointer", fn);
    UC_REQUIRE_DTYPE(fn, dtype, true);
    UC_REQUIRE(B > 0 && T > 0 && C > 0, "%s: bad shape B=%lld T=%lld C=%lld", fn, (long long)B, (long long)T, (long long)C);
    UC_REQUIRE(ld >= C, "%s: ld (%lld) < C (%lld)", fn, (long long)ld, (long long)C);
    const int V = pool_vec(dtype);
    UC_REQUIRE((uintptr_t)x % 16 == 0 && ld % V == 0, "%s: x must be 16-byte aligned with ld a multiple of %d (16-byte rows)", fn, V);
    UC_REQUIRE((uintptr_t)out % 4 == 0 && (uintptr_t)ws % 4 == 0, "%s: out / ws must be 4-byte aligned", fn);
    const int64_t nchunk = pool_chunks(T);
    const int64_t colblocks = ((C + V - 1) / V + 63) / 64;
    const int64_t total = B * C;
    UC_REQUIRE(B <= 65535 && nchunk <= 65535 && C <= 0x7fffffff && (total + 255) / 256 <= 0x7fffffff,
               "%s: grid limit exceeded (B <= 65535, T <= %d, C < 2^31, B * C < 2^39)", fn, 65535 * POOL_CHUNK);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)colblocks, (unsigned)nchunk, (unsigned)B), block(64 * POOL_WAVES);
    UC_DISPATCH_F16(fn, dtype, hipLaunchKernelGGL(token_pool_partial_kernel<Tag>, grid, block, 0, st, (const Tag::storage*)x, ld, ws, (int)T, (int)C, (int)nchunk));
    UC_CHECK_LAUNCH(fn);
    hipLaunchKernelGGL(token_pool_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const float*)ws, out, total, (int)T,
                       (int)C, (int)nchunk);
    UC_CHECK_LAUNCH(fn);
    return UC_OK;
}

extern "C" int uc_token_pool_bwd(const float* g, const void* gate, int64_t ld_gate, void* out, int64_t ld_out, int dtype, int64_t B,
                                 int64_t T, int64_t C, uc_stream_t stream) {
    const char* fn = "uc_token_pool_bwd";
    UC_REQUIRE(g && out, "%s: null pointer", fn);
    UC_REQUIRE_DTYPE(fn, dtype, true);
    UC_REQUIRE(B > 0 && T > 0 && C > 0, "%s: bad shape B=%lld T=%lld C=%lld", fn, (long long)B, (long long)T, (long long)C);
    UC_REQUIRE(ld_out >= C, "%s: ld_out (%lld) < C (%lld)", fn, (long long)ld_out, (long long)C);
    UC_REQUIRE(!gate || ld_gate >= C, "%s: ld_gate (%lld) < C (%lld)", fn, (long long)ld_gate, (long long)C);
    const int V = pool_vec(dtype);
    UC_REQUIRE((uintptr_t)g % 4 == 0 && (uintptr_t)out % 16 == 0 && ld_out % V == 0,
               "%s: out must be 16-byte aligned with ld_out a multiple of %d (16-byte rows), g 4-byte aligned", fn, V);
    UC_REQUIRE(!gate || ((uintptr_t)gate % 16 == 0 && ld_gate % V == 0), "%s: gate must be 16-byte aligned with ld_gate a multiple of %d", fn, V);
    const int64_t ngroups = (C + V - 1) / V;
    UC_REQUIRE(T <= 0x7fffffff && C <= 0x7fffffff && B * T <= ((int64_t)1 << 40) / ngroups && (B * T * ngroups + 255) / 256 <= 0x7fffffff,
               "%s: grid limit exceeded (T, C < 2^31, B * T * ceil(C / %d) < 2^39)", fn, V);
    const int64_t total = B * T * ngroups;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((total + 255) / 256)), block(256);
    UC_DISPATCH_F16(fn, dtype, hipLaunchKernelGGL(token_pool_bwd_kernel<Tag>, grid, block, 0, st, g, (const Tag::storage*)gate, ld_gate, (Tag::storage*)out, ld_out, total,
                                                  (int)T, (int)C, (int)ngroups));
    UC_CHECK_LAUNCH(fn);
    return UC_OK;
}
