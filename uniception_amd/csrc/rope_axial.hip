// Axial RoPE of the DINOv3 ViT, in place on q | k of a packed projection (gfx950).  An HBM-bound streaming kernel like rope2d_kernel
// (rope_norm.hip): one read and one write of the rotated operands, 16-byte accesses per lane where the layout allows.
//
// Arithmetic (published DINOv3 `rope_apply` / transformers modeling_dinov3_vit.py apply_rotary_pos_emb + rotate_half):
//   Q = D/4; a head's channels are [y | x | y | x], each Q wide; channel j is paired with j + D/2.
//   token n >= prefix lies at (y, x) = ((n - prefix) / grid_w, (n - prefix) % grid_w)
//   pair (j, j + 2Q)         : (c, s) = table_y[y][j]        u' = u c - v s,  v' = v c + u s
//   pair (Q + j, Q + j + 2Q) : (c, s) = table_x[x][j]        (inverse: s negated — the gradient path)
//   tokens [0, prefix) — the class and register tokens — are not touched.
// The kernel computes no trigonometry: the host builds the two tables (in fp32, in the reference's order of operations), so the
// coordinates may be anything — normalised patch centres, per axis, augmented per call in training.
// Work split: a workgroup owns TOK consecutive tokens of the B*N.  Phase 1 copies their (cos, sin) rows into LDS; phase 2 streams
// every part (q, k) and every head of those tokens through them.
#include "vec_access.h"

#define UC_ROPE_AXIAL_TOK 8

template <typename Tag, bool VEC8>
__global__ __launch_bounds__(256) void rope_axial_kernel(typename Tag::storage* __restrict__ tok, const float2* __restrict__ table_y,
                                                         const float2* __restrict__ table_x, int64_t BN, int N, int H, int Q,
                                                         int64_t sb, int64_t sn, int64_t sh, int parts, int64_t sp, int prefix,
                                                         int grid_w, float sgn) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float2* cs = reinterpret_cast<float2*>(smem_raw);  // [TOK][2][Q]
    const int64_t tok0 = (int64_t)blockIdx.x * UC_ROPE_AXIAL_TOK;
    const int ntok = (int)min((int64_t)UC_ROPE_AXIAL_TOK, BN - tok0);
    const int tab = ntok * 2 * Q;
    for (int t = threadIdx.x; t < tab; t += blockDim.x) {
        const int i = t % Q;
        const int axis = (t / Q) & 1;
        const int lt = t / (2 * Q);
        const int p = (int)((tok0 + lt) % N) - prefix;
        if (p < 0) continue;           // a prefix token: its rows are never read
        const float2 k = axis ? table_x[(int64_t)(p % grid_w) * Q + i] : table_y[(int64_t)(p / grid_w) * Q + i];
        cs[t] = make_float2(k.x, sgn * k.y);
    }
    __syncthreads();
    constexpr int VEC = VEC8 ? 8 : 1;
    const int qv = Q / VEC;                // work items per quarter of a head
    const int per_part = H * 2 * qv;
    const int per_tok = parts * per_part;
    const int items = ntok * per_tok;
    for (int it = threadIdx.x; it < items; it += blockDim.x) {
        const int g = it % qv;
        const int axis = (it / qv) & 1;
        const int h = (it / (2 * qv)) % H;
        const int part = (it / per_part) % parts;
        const int lt = it / per_tok;
        const int64_t t = tok0 + lt;
        const int64_t b = t / N, n = t % N;
        if (n < prefix) continue;
        typename Tag::storage* pu = tok + (int64_t)part * sp + b * sb + n * sn + (int64_t)h * sh + axis * Q + g * VEC;
        typename Tag::storage* pv = pu + 2 * Q;
        const float2* c = cs + (lt * 2 + axis) * Q + g * VEC;
        if constexpr (VEC8) {
            Vec8 u = vec_load8<Tag>(pu), v = vec_load8<Tag>(pv), ou, ov;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float2 k = c[e];
                ou.v[e] = u.v[e] * k.x - v.v[e] * k.y;
                ov.v[e] = v.v[e] * k.x + u.v[e] * k.y;
            }
            vec_store8<Tag>(pu, ou);
            vec_store8<Tag>(pv, ov);
        } else {
            const float u = Tag::load(pu), v = Tag::load(pv);
            const float2 k = c[0];
            Tag::store(pu, u * k.x - v * k.y);
            Tag::store(pv, v * k.x + u * k.y);
        }
    }
}

template <typename Tag>
static void launch_rope_axial(void* tokens, const float* table_y, const float* table_x, int64_t BN, int N, int H, int Q, int64_t sb,
                              int64_t sn, int64_t sh, int parts, int64_t sp, int prefix, int grid_w, float sgn, hipStream_t st) {
    typedef typename Tag::storage S;
    const size_t smem = (size_t)UC_ROPE_AXIAL_TOK * 2 * Q * sizeof(float2);
    const unsigned grid = (unsigned)ceil_div64(BN, UC_ROPE_AXIAL_TOK);
    // 16-byte accesses: eight channels of a quarter per work item, every address 16-byte aligned; else element by element
    const int64_t al = 16 / (int64_t)sizeof(S);
    const bool vec8 = (Q % 8 == 0) && (sb % al == 0) && (sn % al == 0) && (sh % al == 0) && (parts == 1 || sp % al == 0) &&
                      ((uintptr_t)tokens % 16 == 0);
    if (vec8)
        hipLaunchKernelGGL((rope_axial_kernel<Tag, true>), dim3(grid), dim3(256), smem, st, (S*)tokens, (const float2*)table_y,
                           (const float2*)table_x, BN, N, H, Q, sb, sn, sh, parts, sp, prefix, grid_w, sgn);
    else
        hipLaunchKernelGGL((rope_axial_kernel<Tag, false>), dim3(grid), dim3(256), smem, st, (S*)tokens, (const float2*)table_y,
                           (const float2*)table_x, BN, N, H, Q, sb, sn, sh, parts, sp, prefix, grid_w, sgn);
}

extern "C" int uc_rope_axial(void* tokens, int B, int N, int H, int D, int64_t sb, int64_t sn, int64_t sh, int parts, int64_t sp,
                             int prefix, int grid_h, int grid_w, const float* table_y, const float* table_x, int inverse, int dtype,
                             uc_stream_t stream) {
    UC_REQUIRE_DTYPE("uc_rope_axial", dtype, true);
    UC_REQUIRE(B >= 0 && N >= 0 && H >= 0 && D > 0, "uc_rope_axial: negative dimension (B=%d N=%d H=%d D=%d)", B, N, H, D);
    UC_REQUIRE(D % 8 == 0, "uc_rope_axial: head_dim must be a multiple of 8 (got %d)", D);
    UC_REQUIRE(D <= 1024, "uc_rope_axial: head_dim %d too large (at most 1024)", D);
    UC_REQUIRE(parts == 1 || parts == 2, "uc_rope_axial: parts must be 1 or 2 (got %d)", parts);
    UC_REQUIRE(prefix >= 0 && grid_h >= 0 && grid_w >= 0 && (int64_t)N == (int64_t)prefix + (int64_t)grid_h * grid_w,
               "uc_rope_axial: N=%d is not prefix + grid_h * grid_w = %d + %d * %d", N, prefix, grid_h, grid_w);
    UC_REQUIRE((int64_t)parts * H * D < ((int64_t)1 << 27), "uc_rope_axial: parts * H * D = %lld too large", (long long)parts * H * D);
    UC_REQUIRE(sb >= 0 && sn >= 0 && sh >= 0 && sp >= 0, "uc_rope_axial: negative stride");
    UC_REQUIRE(table_y && table_x, "uc_rope_axial: null table");
    UC_REQUIRE((uintptr_t)table_y % 8 == 0 && (uintptr_t)table_x % 8 == 0, "uc_rope_axial: the tables must be 8-byte aligned");
    if ((int64_t)B * N * H == 0 || (int64_t)grid_h * grid_w == 0) return UC_OK;
    UC_REQUIRE(tokens, "uc_rope_axial: null pointer");
    const float sgn = inverse ? -1.f : 1.f;
    hipStream_t st = (hipStream_t)stream;
    UC_DISPATCH_F16("uc_rope_axial", dtype, launch_rope_axial<Tag>(tokens, table_y, table_x, (int64_t)B * N, N, H, D / 4, sb, sn, sh, parts, sp,
                                                                  prefix, grid_w, sgn, st));
    UC_CHECK_LAUNCH("uc_rope_axial");
    return UC_OK;
}
