#pragma once
// Epilogues of the direct-to-LDS GEMM kernels (gemm_glds_kernel.h): operand and activation helpers, the bounce helpers, the eight
// glds_epilogue_* families and glds_epilogue_dispatch, which picks the family a wave's accumulator block drains through.  Every kernel
// calls glds_epilogue_dispatch once per accumulator block, behind the barrier that frees its LDS image for the bounce space.
#include "mma_tile.h"
#include "gemm_glds.h"
#include "knobs.h"
#include <stdlib.h>

// How the epilogues see the kernel parameters: through the kernarg segment (scalar loads at the point of use), see the
// kernel's epilogue section.
#if defined(__HIP_DEVICE_COMPILE__)
typedef const __attribute__((opencl_constant)) GldsParams& glds_pe_t;
#else
typedef const GldsParams& glds_pe_t;
#endif
#include <algorithm>
#include <type_traits>

// fp16 operand form (F16 = true): the same kernels with v_mfma_f32_16x16x32_f16 and fp16 stores — the prediction heads'
// "TF32-class" mode (10-bit mantissa like TF32, which is what the reference's fp32 heads run on under allow_tf32,
// libs/croco/blocks.py:15 / factory/dust3r.py:288-309), at the bf16 rate.  Only the EPI_ALL family is instantiated for it (3x3
// convolutions, 1x1 convolutions / ConvTranspose GEMMs: bias, ReLU / GELU, residuals, fused tail); RoPE / VT / LayerNorm options
// are rejected by the launcher.
template <bool F16>
__device__ __forceinline__ float4_t glds_mfma(bf16x8_t a, bf16x8_t b, float4_t c) {
    if constexpr (F16) return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
template <bool F16>
__device__ __forceinline__ unsigned glds_pack2(float lo, float hi) {
    if constexpr (F16) {
        const float2v_t v = {uc_sat_f16(lo), uc_sat_f16(hi)};      // (saturating: see common.h)
        return __builtin_bit_cast(unsigned, __builtin_convertvector(v, half2v_t));
    } else return pack_bf16x2(lo, hi);
}
__device__ __forceinline__ float4_t glds_unpack_f16x4(uint2 q) {
    const float2v_t a = __builtin_convertvector(__builtin_bit_cast(half2v_t, q.x), float2v_t);
    const float2v_t b = __builtin_convertvector(__builtin_bit_cast(half2v_t, q.y), float2v_t);
    return (float4_t){a.x, a.y, b.x, b.y};
}

// erf-GELU of the bf16 MFMA path.  libm's erff is a branchy two-range evaluation (~50 VALU ops per element once both
// sides of the branch run in a wave); with only 16 K-steps per fc1 tile that epilogue cost as much as the MFMA loop.
// Abramowitz-Stegun 7.1.26: erf(z) = 1 - (a1 t + .. + a5 t^5) exp(-z^2), t = 1/(1 + p z), |error| <= 1.5e-7 — at fp32
// rounding level and three orders below the bf16 output's own rounding.  (The fp32 verification kernel keeps erff.)
__device__ __forceinline__ float glds_gelu(float x) {
    const float z = fabsf(x) * 0.70710678118654752440f;
    const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, z, 1.0f));
    float poly = fmaf(1.061405429f, t, -1.453152027f);
    poly = fmaf(poly, t, 1.421413741f);
    poly = fmaf(poly, t, -0.284496736f);
    poly = fmaf(poly, t, 0.254829592f);
    const float e = __builtin_amdgcn_exp2f(-z * z * 1.44269504088896340736f);
    const float erf_abs = fmaf(-poly * t, e, 1.0f);            // erf(|x|/sqrt2)
    const float erf_s = __builtin_copysignf(erf_abs, x);
    return 0.5f * x * (1.0f + erf_s);
}
// d/dx of the activation at pre-activation x: GELU' = Phi(x) + x phi(x); ReLU' = [x > 0]
__device__ __forceinline__ float glds_dact(float x, int act) {
    if (act == UC_ACT_RELU) return x > 0.f ? 1.f : 0.f;
    const float z = fabsf(x) * 0.70710678118654752440f;
    const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, z, 1.0f));
    float poly = fmaf(1.061405429f, t, -1.453152027f);
    poly = fmaf(poly, t, 1.421413741f);
    poly = fmaf(poly, t, -0.284496736f);
    poly = fmaf(poly, t, 0.254829592f);
    const float e = __builtin_amdgcn_exp2f(-z * z * 1.44269504088896340736f);      // exp(-x^2/2)
    const float erf_s = __builtin_copysignf(fmaf(-poly * t, e, 1.0f), x);
    return fmaf(0.5f, erf_s, 0.5f) + x * e * 0.39894228040143267794f;
}
__device__ __forceinline__ float glds_act(float v, int act) {
    if (act == UC_ACT_GELU_ERF) return glds_gelu(v);
    if (act == UC_ACT_RELU) return fmaxf(v, 0.f);
    return v;
}

// chunk swizzle key of LDS row r: 128-B rows (r>>1)&7, 64-B rows 3*((r>>2)&1) — both make the ds_read_b128 fragment
// loads (lane = row, lane>>4 = k chunk) conflict-free within the hardware's 16-lane service groups
template <int BK_>
__device__ __forceinline__ int glds_swz(int r) { return BK_ == 64 ? ((r >> 1) & 7) : (((r >> 2) & 1) * 3); }

// Side panel of the eight-wave kernel (GldsParams::side_lds): 8 KiB of LDS behind the two-stage ring, filled by one DMA piece per wave
// before the first K-step — (mean, rstd) of the tile's 256 rows, column sums and bias of its 256 columns, RoPE positions of its rows.
constexpr int GLDS_SIDE_STATS = 0, GLDS_SIDE_COLSUM = 2048, GLDS_SIDE_BIAS = 3072, GLDS_SIDE_POS = 4096, GLDS_SIDE_BYTES = 8192;

// (mean, rstd) of row m for the folded-LayerNorm epilogues: finalized by uc_ln_stats_finalize, or merged here from the producer's
// block partials (small batches)
template <bool BATCH = false>
__device__ __forceinline__ float2 glds_ln_row_stats(glds_pe_t p, int64_t m) {
    if (p.ln_partial) return uc_ln_merge_row<BATCH>(p.ln_partial + m, p.M, p.ln_nblk, p.ln_eps);      // partials are [nblk][M]
    return p.ln_stats[m];
}

// Epilogue of V tiles that are written in the packed VT layout (un-swapped orientation).
template <int FA, bool LN = false, bool BATCH = false>
__device__ __forceinline__ void glds_epilogue_vt(glds_pe_t p, float4_t (&acc)[FA][4], int64_t wave_m, int64_t wave_n, int lane,
                                                 char* wbuf, const char* side = nullptr) {
    const int frow = lane & 15;
    const int g = lane >> 4;
    // Folded LayerNorm (LN): value = rstd[row] * (acc - mean[row] * colsum[channel]) + bias[channel], rows 16 i + 4 g + r,
    // channel 16 j + frow.  Lane l holds the statistics of row l (one coalesced load); the four rows of a fragment come
    // through ds_bpermute.  The correction is applied where a value is consumed: rewriting the 64 accumulators in place
    // first made the compiler park all of them in scratch.
    float csj[4] = {0.f, 0.f, 0.f, 0.f};
    float2 mine = make_float2(0.f, 1.f);
    static_assert(!LN || FA == 4, "folded LayerNorm: 64-row wave tiles");
    if constexpr (LN) {
#pragma unroll
        for (int j = 0; j < 4; ++j) csj[j] = side ? reinterpret_cast<const float*>(side + GLDS_SIDE_COLSUM)[(int)(wave_n & 255) + 16 * j + frow]
                                                  : p.ln_colsum[wave_n + 16 * j + frow];
        mine = side ? reinterpret_cast<const float2*>(side + GLDS_SIDE_STATS)[(int)(wave_m & 255) + lane]
                    : glds_ln_row_stats<BATCH>(p, min(wave_m + lane, p.M - 1));
    }
    auto bias_of = [&](int j) __attribute__((always_inline)) -> float {
        if (side) return reinterpret_cast<const float*>(side + GLDS_SIDE_BIAS)[(int)(wave_n & 255) + 16 * j + frow];     // (side panel: bias present, launcher-checked)
        return p.bias ? p.bias[wave_n + 16 * j + frow] : 0.f;
    };
    float mu[4] = {0.f, 0.f, 0.f, 0.f}, rs[4] = {1.f, 1.f, 1.f, 1.f};
    auto row_stats = [&](int i) __attribute__((always_inline)) {
        if constexpr (LN) {
#pragma unroll
            for (int r = 0; r < 4; ++r) { mu[r] = __shfl(mine.x, 16 * i + 4 * g + r, 64); rs[r] = __shfl(mine.y, 16 * i + 4 * g + r, 64); }
        }
    };
    auto val = [&](int i, int j, int r, float bc) __attribute__((always_inline)) -> float {
        if constexpr (LN) return __builtin_fmaf(__builtin_fmaf(-mu[r], csj[j], acc[i][j][r]), rs[r], bc);
        else return acc[i][j][r] + bc;
    };
    if (FA == 4 && (p.vt_ntok & 63) == 0 && wave_m + 64 <= p.M && ((uintptr_t)p.vt_out & 15) == 0 && !UC_DBG(p, 16)) {
        // The wave's 64 tokens are one aligned 64-position group of one image: 64 channel rows x 128 contiguous bytes of VT.
        // Bounce [channel d][position] through the wave's LDS block (chunk c of row d at chunk c ^ (d & 7), 8-byte halves
        // swapped when d & 8) and store whole rows: 8 x dwordx4 instead of 16 x dwordx2 that touch 16 rows x 32 B each.
        const int head = (int)((wave_n - p.vt_col0) >> 6);
        const int nheads = (int)((p.N - p.vt_col0) >> 6);
        float bcj[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) bcj[j] = bias_of(j);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            row_stats(i);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int d = 16 * j + frow;
                const uint2 pk = (uint2){pack_bf16x2(val(i, j, 0, bcj[j]), val(i, j, 1, bcj[j])), pack_bf16x2(val(i, j, 2, bcj[j]), val(i, j, 3, bcj[j]))};
                *reinterpret_cast<uint2*>(wbuf + d * 128 + (((2 * i + (g & 1)) ^ (d & 7)) << 4) + (((g >> 1) ^ ((d >> 3) & 1)) << 3)) = pk;
            }
        }
        const int b = (int)(wave_m / p.vt_ntok);
        const int tok0 = (int)(wave_m - (int64_t)b * p.vt_ntok);
        bf16_t* base = p.vt_out + ((int64_t)b * nheads + head) * 64 * (int64_t)p.vt_npad + tok0;
        const int crow = lane >> 3, pch = lane & 7;
#pragma unroll
        for (int ps = 0; ps < 8; ++ps) {
            const int d = 8 * ps + crow;
            uint4 v = *reinterpret_cast<const uint4*>(wbuf + d * 128 + (pch << 4));
            if (ps & 1) v = (uint4){v.z, v.w, v.x, v.y};
            *reinterpret_cast<uint4*>(base + (int64_t)d * p.vt_npad + ((pch ^ (d & 7)) << 3)) = v;
        }
        return;
    }
    {
        // acc[i][j][r]: token row m = wave_m + 16i + 4g + r, channel column wave_n + 16j + frow
        const int head = (int)((wave_n - p.vt_col0) >> 6);
        const int nheads = (int)((p.N - p.vt_col0) >> 6);
        // token counts that are multiples of 4 (round 6: 196 tokens of a 224 x 224 view; before: multiples of 16 only): the four rows
        // mb .. mb + 3 of a lane (mb is a multiple of 4) are one image's aligned token quad, i.e. four CONSECUTIVE positions of the
        // permuted 16-key group — one 8-byte store per channel, four lanes filling 32 contiguous bytes of a channel row, instead of
        // sixteen 2-byte stores (the 224 x 224 forward's QKV / KV GEMMs ran at 0.21-0.31 of peak on that path)
        const bool aligned = (p.vt_ntok & 3) == 0;
        float bcol[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) bcol[j] = bias_of(j);
#pragma unroll
        for (int i = 0; i < FA; ++i) {
            const int64_t mb = wave_m + 16 * i + 4 * g;
            row_stats(i);
            if (aligned) {
                if (mb >= p.M) continue;
                const int b = (int)(mb / p.vt_ntok);
                const int tok = (int)(mb % p.vt_ntok);
                const int qi = (tok & 15) >> 2;                      // the quad's index inside its 16-key group (uc_vt_perm)
                const int pos = (tok & ~15) + ((qi & 1) << 3) + ((qi >> 1) << 2);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int d = 16 * j + frow;
                    bf16_t* dst = p.vt_out + (((int64_t)b * nheads + head) * 64 + d) * p.vt_npad + pos;
                    uint2 pk;
                    pk.x = pack_bf16x2(val(i, j, 0, bcol[j]), val(i, j, 1, bcol[j]));
                    pk.y = pack_bf16x2(val(i, j, 2, bcol[j]), val(i, j, 3, bcol[j]));
                    *reinterpret_cast<uint2*>(dst) = pk;
                }
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int64_t m = mb + r;
                    if (m >= p.M) continue;
                    const int b = (int)(m / p.vt_ntok);
                    const int tok = (int)(m % p.vt_ntok);
                    const int w = tok & 15;
                    const int pos = (tok & ~15) + (((w >> 2) & 1) << 3) + (w & 3) + ((w >> 3) << 2);
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        p.vt_out[(((int64_t)b * nheads + head) * 64 + 16 * j + frow) * p.vt_npad + pos] =
                            f32_to_bf16(val(i, j, r, bcol[j]));
                }
            }
        }
    }
}

// Epilogue of the swapped orientation (bias -> activation -> fused RoPE-2D -> residual(s) -> dact -> store).
//
// In the accumulator layout one store instruction touches 16 rows x 32-64 B, and the vector memory path retires about
// one row segment per 4 cycles per CU whatever its width: a 256x256 tile's store tail took 7 us (bf16 or fp32 output,
// tools/probes/store_tail.hip) against 1-2 us when every instruction covers whole 128-B lines.  So each wave bounces its
// 16x64 fragment rows through a private, XOR-swizzled 4-KiB LDS block (the stage buffers are free after the K-loop)
// and does all global traffic — pre-activation copy, residual reads, dact reads, the store — with a lane owning 4
// consecutive columns and 16 lanes covering one row (4 rows x 256 B of fp32 or 4 x 128 B of bf16 per instruction).
// Bias/activation move to that layout too; RoPE (partner channels live in one lane of the accumulator layout) is
// applied before the bounce.
//
// Run-time option tests must not sit inside per-element code: a `p.act` test per value compiled into a scalar compare
// and branch per ELEMENT (the epilogue then cost as much as six K-steps, half of it instruction fetch: the kernel was
// 40 k lines of ISA).  The two shapes that carry the forward are specialised at compile time —
//   glds_epilogue_bf16: bf16 output, no residual (qkv, fc1, kv projections, every convolution), ACT a template parameter,
//                       bf16 bounce;
//   glds_epilogue_fast<.., KIND 1>: fp32 output added to one or two fp32 residual streams (proj, fc2), fp32 bounce
//                       (its KIND 0 form is the fp32-bounce variant of the bf16 store, kept for A/B runs);
// everything else (split-K slabs, pre-activation copies, dact, bf16 residuals, partial column blocks, unaligned
// operands) takes a rolled generic drain whose option tests are per 4-column group.
// erf-GELU of the bf16-store epilogues without transcendentals: GELU(x) = x Phi(x), Phi(x) - 1/2 = x_c Q(x_c^2) with x_c = x clamped
// to +-4.5 and Q a degree-10 polynomial (least-squares fit in the Chebyshev basis over [0, 4.5^2], evaluated by Horner in
// t = 2 x_c^2 / 4.5^2 - 1).  |error| <= 1.2e-5 absolute inside the clamp, <= 3e-5 beyond it (Phi(-4.5) = 3.4e-6 instead of -> 0)
// — two orders below the bf16 output's own rounding.  15 packed-fp32-able operations per element instead of 16 scalar ones plus
// an exp2 and a reciprocal on the quarter-rate transcendental unit: the GELU epilogue of fc1 cost 7.9 us per 256x256 tile
// (as much as five K-steps), the VALU being the only unit at work in an epilogue.
// Explicit fused multiply-adds for the epilogue arithmetic: left to `-ffp-contract`, hipcc contracts each unrolled copy of an
// expression its own way, and a row's bf16 roundings would depend on where in a tile (or in a batch) the row sits.
__device__ __forceinline__ float4_t glds_fma4(float4_t a, float4_t b, float4_t c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ float4_t glds_splat4(float v) { return (float4_t){v, v, v, v}; }

__device__ __forceinline__ float4_t glds_gelu4(float4_t x) {
    float4_t xc;
#pragma unroll
    for (int r = 0; r < 4; ++r) xc[r] = __builtin_amdgcn_fmed3f(x[r], -4.5f, 4.5f);
    const float4_t t = glds_fma4(xc * xc, glds_splat4(2.0f / 20.25f), glds_splat4(-1.0f));
    float4_t q = glds_fma4(t, glds_splat4(8.660091177e-04f), glds_splat4(-2.253821881e-03f));
    q = glds_fma4(q, t, glds_splat4(2.972107097e-03f));
    q = glds_fma4(q, t, glds_splat4(-5.424589433e-03f));
    q = glds_fma4(q, t, glds_splat4(1.124217992e-02f));
    q = glds_fma4(q, t, glds_splat4(-1.890690569e-02f));
    q = glds_fma4(q, t, glds_splat4(2.834482012e-02f));
    q = glds_fma4(q, t, glds_splat4(-4.013649033e-02f));
    q = glds_fma4(q, t, glds_splat4(5.469475207e-02f));
    q = glds_fma4(q, t, glds_splat4(-7.719214694e-02f));
    q = glds_fma4(q, t, glds_splat4(1.569050361e-01f));
    return x * glds_fma4(xc, q, glds_splat4(0.5f));
}

template <int ACT>
__device__ __forceinline__ float4_t glds_act4(float4_t v) {
    if constexpr (ACT == UC_ACT_GELU_ERF) return glds_gelu4(v);
    else if constexpr (ACT == UC_ACT_RELU) { for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f); return v; }
    else return v;
}

template <int ACT>
__device__ __forceinline__ float glds_act_c(float v) {
    if constexpr (ACT == UC_ACT_GELU_ERF) return glds_gelu(v);
    else if constexpr (ACT == UC_ACT_RELU) return fmaxf(v, 0.f);
    else return v;
}

// LDS bounce block of one wave: 16 rows x 256 B, 16-B chunk c of row r stored at chunk c ^ r (conflict-free for the
// accumulator-layout ds_write_b128 and the row-contiguous ds_read_b128 alike)
__device__ __forceinline__ void glds_bounce_write(char* buf, int frow, int g, int j, float4_t v) {
    *reinterpret_cast<float4_t*>(buf + frow * 256 + (((4 * j + g) ^ frow) << 4)) = v;
}
__device__ __forceinline__ float4_t glds_bounce_read(const char* buf, int R, int cchunk) {
    return *reinterpret_cast<const float4_t*>(buf + R * 256 + ((cchunk ^ R) << 4));
}

// accumulator rows of fragment row-block i (+ bias and RoPE for mode 1) -> bounce block
template <int FA>
__device__ __forceinline__ void glds_stage_rows(glds_pe_t p, float4_t (&acc)[FA][4], int i, int mode, int64_t wave_m,
                                                int64_t wave_n, int frow, int g, char* buf) {
    if (mode == 1) {
        const int64_t m = min(wave_m + 16 * i + frow, p.M - 1);
        int py = (int)p.rope_pos[m * 2 + 0];
        int px = (int)p.rope_pos[m * 2 + 1];
        py = min(max(py, 0), p.rope_npos - 1);
        px = min(max(px, 0), p.rope_npos - 1);
#pragma unroll
        for (int h = 0; h < 2; ++h) {      // fragment pair (2h, 2h+1) = channels d, d+16 of the y (h = 0) / x (h = 1) half
            const float4_t* tb = reinterpret_cast<const float4_t*>(p.rope_table + (h ? px : py) * 16 + 4 * g);
            const float4_t c0 = tb[0], c1 = tb[1];                               // (cos,sin) x 4
            const float cs[4] = {c0.x, c0.z, c1.x, c1.z}, sn[4] = {c0.y, c0.w, c1.y, c1.w};
            float4_t bu = (float4_t){0.f, 0.f, 0.f, 0.f}, bw = bu;
            if (p.bias) {                  // rope tiles are whole 64-column heads inside N (launcher-checked), bias 16-B aligned or scalar
                const float* bp = p.bias + wave_n + 32 * h + 4 * g;
                bu = (float4_t){bp[0], bp[1], bp[2], bp[3]};
                bw = (float4_t){bp[16], bp[17], bp[18], bp[19]};
            }
            float4_t ou, ow;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float u = acc[i][2 * h][r] + bu[r], w = acc[i][2 * h + 1][r] + bw[r];   // no activation with RoPE (launcher-checked)
                ou[r] = u * cs[r] - w * sn[r];
                ow[r] = w * cs[r] + u * sn[r];
            }
            glds_bounce_write(buf, frow, g, 2 * h, ou);
            glds_bounce_write(buf, frow, g, 2 * h + 1, ow);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) glds_bounce_write(buf, frow, g, j, acc[i][j]);
    }
}

template <int FA, int ACT, int KIND, bool NT = false>
__device__ __forceinline__ void glds_epilogue_fast(glds_pe_t p, float4_t (&acc)[FA][4], int mode, int64_t wave_m,
                                                   int64_t wave_n, int lane, char* wbuf) {
    const int frow = lane & 15, g = lane >> 4;
    // drain layout.  KIND 0 (bf16 out): a lane owns 8 consecutive columns, 8 lanes cover a row, an instruction stores 8
    // rows x 128 B as dwordx4.  KIND 1 (fp32): 4 columns per lane, 16 lanes per row, 4 rows x 256 B per instruction.
    constexpr int LPR = KIND == 0 ? 8 : 16;              // lanes per row
    constexpr int RPP = 64 / LPR;                        // rows per pass
    constexpr int NPS = 16 / RPP;                        // passes per 16-row block
    const int crow = lane / LPR, cc = lane % LPR;
    const int64_t nb = wave_n + (KIND == 0 ? 8 : 4) * cc;
    float4_t bias4 = (float4_t){0.f, 0.f, 0.f, 0.f}, bias4b = bias4;
    if (mode != 1 && p.bias) {
        bias4 = *reinterpret_cast<const float4_t*>(p.bias + nb);
        if constexpr (KIND == 0) bias4b = *reinterpret_cast<const float4_t*>(p.bias + nb + 4);
    }
    const int rows_left = (int)min((int64_t)(16 * FA), p.M - wave_m) - crow;      // row 16i + RPP*ps + crow exists iff 16i + RPP*ps < rows_left
    constexpr int ESZ = KIND == 0 ? 2 : 4;
    char* cp = (char*)p.C + ((wave_m + crow) * p.ldc + nb) * ESZ;
    const int64_t cstep = RPP * p.ldc * ESZ;
    const char* rp = nullptr; const char* rp2 = nullptr; int64_t rstep = 0;
    if constexpr (KIND == 1) {
        rp = (const char*)p.residual + ((wave_m + crow) * p.ldr + nb) * 4;
        rp2 = p.residual2 ? (const char*)p.residual2 + ((wave_m + crow) * p.ldr + nb) * 4 : nullptr;
        rstep = RPP * p.ldr * 4;
    }
    // the next row block is staged before the current one is drained: its LDS writes overlap this block's global traffic
    glds_stage_rows<FA>(p, acc, 0, mode, wave_m, wave_n, frow, g, wbuf);
#pragma unroll
    for (int i = 0; i < FA; ++i) {
        const char* buf = wbuf + (i & 1) * 4096;
        if (i + 1 < FA) glds_stage_rows<FA>(p, acc, i + 1, mode, wave_m, wave_n, frow, g, wbuf + ((i + 1) & 1) * 4096);
#pragma unroll
        for (int ps = 0; ps < NPS; ++ps) {
            const int R = RPP * ps + crow;
            if constexpr (KIND == 0) {
                float4_t v = glds_bounce_read(buf, R, 2 * cc), w = glds_bounce_read(buf, R, 2 * cc + 1);
                if (16 * i + RPP * ps < rows_left) {
                    if (mode != 1) {
                        v += bias4; w += bias4b;
#pragma unroll
                        for (int r = 0; r < 4; ++r) { v[r] = glds_act_c<ACT>(v[r]); w[r] = glds_act_c<ACT>(w[r]); }
                    }
                    *reinterpret_cast<uint4*>(cp) = (uint4){pack_bf16x2(v.x, v.y), pack_bf16x2(v.z, v.w), pack_bf16x2(w.x, w.y), pack_bf16x2(w.z, w.w)};
                }
            } else {
                float4_t v = glds_bounce_read(buf, R, cc);
                if (16 * i + RPP * ps < rows_left) {
                    if (mode != 1) v += bias4;
                    // NT (outputs of more than 128 MB, half the Infinity Cache): the residual stream is read once and written once per
                    // sub-layer — streaming it keeps the A / W panels of the K-loop in the L2s (+1.2 % on the forward); smaller
                    // outputs (the decoder's) stay cacheable, their consumer (LayerNorm) finds them on chip
                    if constexpr (NT) {
                        v += __builtin_nontemporal_load(reinterpret_cast<const float4_t*>(rp));
                        if (rp2) v += __builtin_nontemporal_load(reinterpret_cast<const float4_t*>(rp2));
                        __builtin_nontemporal_store(v, reinterpret_cast<float4_t*>(cp));
                    } else {
                        v += *reinterpret_cast<const float4_t*>(rp);
                        if (rp2) v += *reinterpret_cast<const float4_t*>(rp2);
                        *reinterpret_cast<float4_t*>(cp) = v;
                    }
                }
            }
            cp += cstep;
            if constexpr (KIND == 1) { rp += rstep; if (rp2) rp2 += rstep; }
        }
    }
}

// sum over the 16 lanes of a DPP row (lanes 16k .. 16k+15), result in every lane
__device__ __forceinline__ float glds_row16_sum(float v) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x121, 0xf, 0xf, false));   // row_ror:1
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x122, 0xf, 0xf, false));   // row_ror:2
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x124, 0xf, 0xf, false));   // row_ror:4
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x128, 0xf, 0xf, false));   // row_ror:8
    return v;
}

// fp32 output, optionally added to an fp32 residual stream (proj, fc2, patch / input embeddings; optionally a second addend).
// The output may alias the residual (in-place accumulate), so the compiler keeps every residual load behind the previous
// store: written as one load -> add -> store chain per 4-row pass that is 16 HBM round trips per wave, 21 us per 256x256
// tile — as long as the K-loop of a K = 1024 GEMM.  Here the residual of row block i + 1 is in flight (4 x 16 B per lane)
// while block i drains; each element is still read before it is written, which is all the in-place form needs.
//
// Producer half of the folded LayerNorm: with p.twin the stored rows are also written as bf16 (the A operand of the next
// GEMM), with p.stats_out every row's (sum, squared deviations from its own mean) over the wave's 64 columns is written
// — the row's 16 lanes reduce with DPP row rotations; uc_ln_stats_finalize merges the blocks into (mean, rstd).
//
// BS (bf16 residual stream, the reference's own policy under autocast): C and the residual(s) are bf16 — 2 + 2 bytes per element
// instead of 4 + 4 + 2; the stored rows ARE the next GEMM's A operand (no twin) and the statistics are those of the ROUNDED values
// the consumer will normalise.
template <int FA, bool NT, bool BS = false>
__device__ __forceinline__ void glds_epilogue_resid(glds_pe_t p, float4_t (&acc)[FA][4], int mode, int64_t wave_m,
                                                    int64_t wave_n, int lane, char* wbuf) {
    constexpr int ES = BS ? 2 : 4;                       // bytes per element of C and of the residual(s)
    const int frow = lane & 15, g = lane >> 4;
    const int crow = lane >> 4, cc = lane & 15;          // drain: 4 columns per lane, 16 lanes per row, 4 rows x 256 B per instruction
    const int64_t nb = wave_n + 4 * cc;
    float4_t bias4 = (float4_t){0.f, 0.f, 0.f, 0.f};
    if (mode != 1 && p.bias) bias4 = *reinterpret_cast<const float4_t*>(p.bias + nb);
    const int rows_left = (int)min((int64_t)(16 * FA), p.M - wave_m) - crow;      // row 16i + 4ps + crow exists iff 16i + 4ps < rows_left
    // wave-uniform 64-bit bases + one 32-bit lane offset per matrix: per-lane 64-bit pointers for C, the residuals, the twin
    // and the statistics cost 10 registers this epilogue does not have (a spill reload between its stores waits for every
    // store issued before it)
    char* cbase = (char*)p.C + (wave_m * p.ldc + wave_n) * ES;
    const unsigned coff = (unsigned)(crow * (int)p.ldc + 4 * cc) * (unsigned)ES;
    const int64_t cstep = 4 * p.ldc * ES;
    // diagnostics (wrong results): dbg & 128 never reads the residual(s), dbg & 256 never writes the twin — together the HBM bytes of
    // a bf16 residual stream (4 per element instead of 10)
    const char* rbase = (p.residual && !UC_DBG(p, 128)) ? (const char*)p.residual + (wave_m * p.ldr + wave_n) * ES : nullptr;
    const char* rbase2 = (p.residual2 && !UC_DBG(p, 128)) ? (const char*)p.residual2 + (wave_m * p.ldr + wave_n) * ES : nullptr;
    const unsigned roff = (unsigned)(crow * (int)p.ldr + 4 * cc) * (unsigned)ES;
    const int64_t rstep = 4 * p.ldr * ES;
    char* tbase = (!BS && p.twin && !UC_DBG(p, 256)) ? (char*)p.twin + (wave_m * p.ldt + wave_n) * 2 : nullptr;
    const unsigned toff = (unsigned)(crow * (int)p.ldt + 4 * cc) * 2u;
    const int64_t tstep = 4 * p.ldt * 2;
    const int nblk = (int)(p.N >> 6);
    float2* sbase = p.stats_out ? p.stats_out + (wave_n >> 6) * p.M + wave_m : nullptr;      // [N/64][M]: block-major (ABI 11)
    (void)nblk;
    // ONE register set for the residual: pass ps of row block i + 1 is requested as soon as pass ps of block i has used
    // its value (each element is still read before the in-place store of its own row), so 4 loads per lane stay in flight.
    // (BS: the four bf16 values stay packed — 2 registers — until they are used; one residual only, see the launcher)
    typedef unsigned glds_u2_t __attribute__((ext_vector_type(2)));
    typedef typename std::conditional<BS, glds_u2_t, float4_t>::type res_t;
    res_t res[4];
    auto load_res = [&](int i, int ps) __attribute__((always_inline)) {
        if constexpr (BS) {
            res[ps] = (glds_u2_t){0u, 0u};
            if (rbase && 16 * i + 4 * ps < rows_left) {
                const glds_u2_t* q = reinterpret_cast<const glds_u2_t*>(rbase + (4 * i + ps) * rstep + roff);
                if constexpr (NT) res[ps] = __builtin_nontemporal_load(q); else res[ps] = *q;
            }
        } else {
            res[ps] = (float4_t){0.f, 0.f, 0.f, 0.f};
            if (rbase && 16 * i + 4 * ps < rows_left) {
                const float4_t* q = reinterpret_cast<const float4_t*>(rbase + (4 * i + ps) * rstep + roff);
                if constexpr (NT) res[ps] = __builtin_nontemporal_load(q); else res[ps] = *q;
                if (rbase2) {
                    const float4_t* q2 = reinterpret_cast<const float4_t*>(rbase2 + (4 * i + ps) * rstep + roff);
                    if constexpr (NT) res[ps] += __builtin_nontemporal_load(q2); else res[ps] += *q2;
                }
            }
        }
    };
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) load_res(0, ps);
    glds_stage_rows<FA>(p, acc, 0, mode, wave_m, wave_n, frow, g, wbuf);
#pragma unroll
    for (int i = 0; i < FA; ++i) {
        const char* buf = wbuf + (i & 1) * 4096;
        if (i + 1 < FA) glds_stage_rows<FA>(p, acc, i + 1, mode, wave_m, wave_n, frow, g, wbuf + ((i + 1) & 1) * 4096);
#pragma unroll
        for (int ps = 0; ps < 4; ++ps) {
            float4_t v = glds_bounce_read(buf, 4 * ps + crow, cc);
            if (mode != 1) v += bias4;
            if constexpr (BS) {
                v += (float4_t){__uint_as_float(res[ps].x << 16), __uint_as_float(res[ps].x & 0xffff0000u), __uint_as_float(res[ps].y << 16),
                                __uint_as_float(res[ps].y & 0xffff0000u)};
            } else v += res[ps];
            if (i + 1 < FA) load_res(i + 1, ps);
            const bool row_ok = 16 * i + 4 * ps < rows_left;
            if constexpr (BS) {
                const glds_u2_t pk = {pack_bf16x2(v.x, v.y), pack_bf16x2(v.z, v.w)};
                if (row_ok) {
                    glds_u2_t* cq = reinterpret_cast<glds_u2_t*>(cbase + (4 * i + ps) * cstep + coff);
                    if constexpr (NT) __builtin_nontemporal_store(pk, cq); else *cq = pk;
                }
                // the statistics below are those of the stored (rounded) row
                v = (float4_t){__uint_as_float(pk.x << 16), __uint_as_float(pk.x & 0xffff0000u), __uint_as_float(pk.y << 16),
                               __uint_as_float(pk.y & 0xffff0000u)};
            } else if (row_ok) {
                // NT (outputs of more than 128 MB, half the Infinity Cache): the residual stream is read once and written once per
                // sub-layer — streaming it keeps the A / W panels of the K-loop in the L2s (+1.2 % on the forward); smaller
                // outputs (the decoder's) stay cacheable, their consumer finds them on chip
                float4_t* cq = reinterpret_cast<float4_t*>(cbase + (4 * i + ps) * cstep + coff);
                if constexpr (NT) __builtin_nontemporal_store(v, cq); else *cq = v;
                if (tbase) *reinterpret_cast<uint2*>(tbase + (4 * i + ps) * tstep + toff) = (uint2){pack_bf16x2(v.x, v.y), pack_bf16x2(v.z, v.w)};
            }
            if (sbase && !UC_DBG(p, 512)) {   // all 64 lanes take part in the row reductions (rows past M carry finite garbage and are not stored)
                // (no FMA contraction here: hipcc contracts each unrolled copy of this block differently, and a row's statistics —
                // hence the bf16 roundings of everything downstream — must not depend on where in a tile the row sits)
#pragma clang fp contract(off)
                const float s = glds_row16_sum((v.x + v.y) + (v.z + v.w));
                const float mu = s * (1.f / 64.f);
                const float4_t dv = v - mu;
                const float q = glds_row16_sum((dv.x * dv.x + dv.y * dv.y) + (dv.z * dv.z + dv.w * dv.w));
                if (row_ok && cc == 0 && !UC_DBG(p, 1024)) sbase[16 * i + 4 * ps + crow] = make_float2(s, q);
            }
        }
    }
}

#ifndef GLDS_BS_RES_AHEAD
#define GLDS_BS_RES_AHEAD 2     // row blocks of residual in flight ahead of the one being drained (bf16-stream epilogue)
#endif
#ifndef GLDS_BS_RES_AHEAD_WIDE
#define GLDS_BS_RES_AHEAD_WIDE 2   // ... in the kernels whose waves own 128-row tiles (eight- and four-wave forms: 256 registers per lane)
#endif
// sum over the 8 lanes 8k .. 8k+7 (one row of the bf16-stream drain), result in every lane: xor 1, xor 2 inside the quad, then the
// mirrored lane of the 8-lane half row (which lies in the other quad)
__device__ __forceinline__ float glds_row8_sum(float v) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xf, 0xf, false));    // quad_perm [1,0,3,2]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xf, 0xf, false));    // quad_perm [2,3,0,1]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xf, 0xf, false));   // row_half_mirror
    return v;
}

// bf16 residual stream (round 4 form): bf16 output = one rounding of acc + bias + bf16 residual, row statistics of the STORED rows.
// Round 3 ran this through the fp32 residual drain (4 columns per lane: 8-byte loads / stores, one scattered 8-byte statistics store
// per row and wave): measured on the encoder's proj GEMM (316 us; 236 with a plain bf16 store) 20 us were the statistics stores
// (1024 eight-byte stores to 1024 different lines per tile), 6 us the reductions, 36 us the residual read (at the HBM burst rate: all
// CUs reach their epilogues together) and 18 us the drain's own instructions.  Here: the bf16-store drain layout — 8 columns per lane,
// 8 lanes per row, 8 rows x 128 B per instruction: 16-byte residual loads and stores, half the instructions; the row sums over 8
// lanes (3 DPP steps instead of 4) of 8 in-lane values; and the statistics leave as ONE coalesced store per 64 rows: after each pass
// every lane of a row holds that row's pair, lane (crow, cc) keeps the pair of pass cc, so at the end lane (crow, cc) owns row
// 8 cc + crow and the 64 lanes write 512 contiguous bytes of the block-major statistics array [N/64][M] (ABI 11).
template <int FA, bool NT>
__device__ __forceinline__ void glds_epilogue_bs(glds_pe_t p, float4_t (&acc)[FA][4], int /*mode*/, int64_t wave_m, int64_t wave_n, int lane,
                                                 char* wbuf) {
    constexpr int mode = 0;      // (the launcher routes no RoPE / VT tile to this family: keeps the RoPE branch of glds_stage_rows out of the kernel)
    const int frow = lane & 15, g = lane >> 4;
    const int crow = lane >> 3, cc = lane & 7;
    const int64_t nb = wave_n + 8 * cc;
    float4_t bias4 = (float4_t){0.f, 0.f, 0.f, 0.f}, bias4b = bias4;
    if (mode != 1 && p.bias) {
        bias4 = *reinterpret_cast<const float4_t*>(p.bias + nb);
        bias4b = *reinterpret_cast<const float4_t*>(p.bias + nb + 4);
    }
    const int rows_total = (int)min((int64_t)(16 * FA), p.M - wave_m);
    const int rows_left = rows_total - crow;              // row 16i + 8ps + crow exists iff 16i + 8ps < rows_left
    // wave-uniform 64-bit bases + one 32-bit lane offset per matrix (see glds_epilogue_resid)
    char* cbase = (char*)p.C + (wave_m * p.ldc + wave_n) * 2;
    const unsigned coff = (unsigned)(crow * (int)p.ldc + 8 * cc) * 2u;
    const int64_t cstep = 8 * p.ldc * 2;
    const char* rbase = (p.residual && !UC_DBG(p, 128)) ? (const char*)p.residual + (wave_m * p.ldr + wave_n) * 2 : nullptr;
    const unsigned roff = (unsigned)(crow * (int)p.ldr + 8 * cc) * 2u;
    const int64_t rstep = 8 * p.ldr * 2;
    float2* sbase = (p.stats_out && !UC_DBG(p, 512)) ? p.stats_out + (wave_n >> 6) * p.M + wave_m : nullptr;
    // the residual of the next AHEAD row blocks (2 x 16 bytes per lane each) is in flight while block i drains
    constexpr int AHEAD = FA > 4 ? GLDS_BS_RES_AHEAD_WIDE : GLDS_BS_RES_AHEAD;
    uint4_t res[AHEAD][2];
    auto load_res = [&](int i, int ps) __attribute__((always_inline)) {
        res[i % AHEAD][ps] = (uint4_t){0u, 0u, 0u, 0u};
        if (rbase && 16 * i + 8 * ps < rows_left) {
            const uint4_t* q = reinterpret_cast<const uint4_t*>(rbase + (2 * i + ps) * rstep + roff);
            if constexpr (NT) res[i % AHEAD][ps] = __builtin_nontemporal_load(q); else res[i % AHEAD][ps] = *q;
        }
    };
    auto lo = [](unsigned u) __attribute__((always_inline)) { return __uint_as_float(u << 16); };
    auto hi = [](unsigned u) __attribute__((always_inline)) { return __uint_as_float(u & 0xffff0000u); };
    float keep_s[FA / 4], keep_q[FA / 4];
#pragma unroll
    for (int h = 0; h < FA / 4; ++h) keep_s[h] = keep_q[h] = 0.f;
#pragma unroll
    for (int i = 0; i < AHEAD && i < FA; ++i) { load_res(i, 0); load_res(i, 1); }
    glds_stage_rows<FA>(p, acc, 0, mode, wave_m, wave_n, frow, g, wbuf);
#pragma unroll
    for (int i = 0; i < FA; ++i) {
        const char* buf = wbuf + (i & 1) * 4096;
        if (i + 1 < FA) glds_stage_rows<FA>(p, acc, i + 1, mode, wave_m, wave_n, frow, g, wbuf + ((i + 1) & 1) * 4096);
#pragma unroll
        for (int ps = 0; ps < 2; ++ps) {
            const int R = 8 * ps + crow;
            float4_t v = glds_bounce_read(buf, R, 2 * cc), w = glds_bounce_read(buf, R, 2 * cc + 1);
            if (mode != 1) { v += bias4; w += bias4b; }
            const uint4_t rr = res[i % AHEAD][ps];
            v += (float4_t){lo(rr.x), hi(rr.x), lo(rr.y), hi(rr.y)};
            w += (float4_t){lo(rr.z), hi(rr.z), lo(rr.w), hi(rr.w)};
            if (i + AHEAD < FA) load_res(i + AHEAD, ps);
            const bool row_ok = 16 * i + 8 * ps < rows_left;
            const uint4_t pk = {pack_bf16x2(v.x, v.y), pack_bf16x2(v.z, v.w), pack_bf16x2(w.x, w.y), pack_bf16x2(w.z, w.w)};
            if (row_ok) {
                uint4_t* cq = reinterpret_cast<uint4_t*>(cbase + (2 * i + ps) * cstep + coff);
                if constexpr (NT) __builtin_nontemporal_store(pk, cq); else *cq = pk;
            }
            if (sbase) {   // statistics of the stored (rounded) row; all 64 lanes take part (rows past M carry finite garbage, not stored)
                // (no FMA contraction: a row's statistics must not depend on where in a tile the row sits — see glds_epilogue_resid)
#pragma clang fp contract(off)
                const float x0 = lo(pk.x), x1 = hi(pk.x), x2 = lo(pk.y), x3 = hi(pk.y), x4 = lo(pk.z), x5 = hi(pk.z), x6 = lo(pk.w), x7 = hi(pk.w);
                const float s = glds_row8_sum(((x0 + x1) + (x2 + x3)) + ((x4 + x5) + (x6 + x7)));
                const float mu = s * (1.f / 64.f);
                const float d0 = x0 - mu, d1 = x1 - mu, d2 = x2 - mu, d3 = x3 - mu, d4 = x4 - mu, d5 = x5 - mu, d6 = x6 - mu, d7 = x7 - mu;
                const float q = glds_row8_sum(((d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3)) + ((d4 * d4 + d5 * d5) + (d6 * d6 + d7 * d7)));
                const bool mine = cc == ((2 * i + ps) & 7);
                keep_s[(2 * i + ps) >> 3] = mine ? s : keep_s[(2 * i + ps) >> 3];
                keep_q[(2 * i + ps) >> 3] = mine ? q : keep_q[(2 * i + ps) >> 3];
            }
        }
    }
    if (sbase && !UC_DBG(p, 1024)) {
#pragma unroll
        for (int h = 0; h < FA / 4; ++h) {
            const int row = 64 * h + 8 * cc + crow;      // pass 8 h + cc covered rows 64 h + 8 cc + (0..7)
            if (row < rows_total) sbase[row] = make_float2(keep_s[h], keep_q[h]);
        }
    }
}

// 16-bit output + bias + one or two 16-bit residuals laid out like C (the residual conv units of the DPT head: conv2(...) + x (+ the
// other path), libs/croco/dpt_block.py:56-63) — the bf16-stream drain above without the statistics, for bf16 or fp16 storage: the
// accumulator rows bounce through LDS in fp32, a lane adds bias and the residuals of its 8 columns in fp32 (16-byte residual loads, the
// next two row blocks' in flight), ONE rounding, 16-byte stores.  Before round 4's last session these launches took the generic drain
// (scalar-ish 8-byte traffic): the same 128^2 256->256 convolution cost 3.48 ms with its two residuals and 2.17 ms without.
template <int FA, bool NT, bool F16>
__device__ __forceinline__ void glds_epilogue_res16(glds_pe_t p, float4_t (&acc)[FA][4], int64_t wave_m, int64_t wave_n, int lane, char* wbuf) {
    const int frow = lane & 15, g = lane >> 4;
    const int crow = lane >> 3, cc = lane & 7;
    const int64_t nb = wave_n + 8 * cc;
    float4_t bias4 = (float4_t){0.f, 0.f, 0.f, 0.f}, bias4b = bias4;
    if (p.bias) {
        bias4 = *reinterpret_cast<const float4_t*>(p.bias + nb);
        bias4b = *reinterpret_cast<const float4_t*>(p.bias + nb + 4);
    }
    const int rows_total = (int)min((int64_t)(16 * FA), p.M - wave_m);
    const int rows_left = rows_total - crow;              // row 16i + 8ps + crow exists iff 16i + 8ps < rows_left
    char* cbase = (char*)p.C + (wave_m * p.ldc + wave_n) * 2;
    const unsigned coff = (unsigned)(crow * (int)p.ldc + 8 * cc) * 2u;
    const int64_t cstep = 8 * p.ldc * 2;
    const char* rbase = (const char*)p.residual + (wave_m * p.ldr + wave_n) * 2;
    const char* r2base = p.residual2 ? (const char*)p.residual2 + (wave_m * p.ldr + wave_n) * 2 : nullptr;
    const unsigned roff = (unsigned)(crow * (int)p.ldr + 8 * cc) * 2u;
    const int64_t rstep = 8 * p.ldr * 2;
    constexpr int AHEAD = 2;
    uint4_t res[AHEAD][2], res2[AHEAD][2];
    auto load_res = [&](int i, int ps) __attribute__((always_inline)) {
        res[i % AHEAD][ps] = (uint4_t){0u, 0u, 0u, 0u};
        res2[i % AHEAD][ps] = (uint4_t){0u, 0u, 0u, 0u};
        if (16 * i + 8 * ps < rows_left) {
            const uint4_t* q = reinterpret_cast<const uint4_t*>(rbase + (2 * i + ps) * rstep + roff);
            if constexpr (NT) res[i % AHEAD][ps] = __builtin_nontemporal_load(q); else res[i % AHEAD][ps] = *q;
            if (r2base) {
                const uint4_t* q2 = reinterpret_cast<const uint4_t*>(r2base + (2 * i + ps) * rstep + roff);
                if constexpr (NT) res2[i % AHEAD][ps] = __builtin_nontemporal_load(q2); else res2[i % AHEAD][ps] = *q2;
            }
        }
    };
    auto add16 = [](float4_t& v, float4_t& w, uint4_t rr) __attribute__((always_inline)) {
        if constexpr (F16) {
            v += glds_unpack_f16x4((uint2){rr.x, rr.y});
            w += glds_unpack_f16x4((uint2){rr.z, rr.w});
        } else {
            v += (float4_t){__uint_as_float(rr.x << 16), __uint_as_float(rr.x & 0xffff0000u), __uint_as_float(rr.y << 16), __uint_as_float(rr.y & 0xffff0000u)};
            w += (float4_t){__uint_as_float(rr.z << 16), __uint_as_float(rr.z & 0xffff0000u), __uint_as_float(rr.w << 16), __uint_as_float(rr.w & 0xffff0000u)};
        }
    };
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < AHEAD && i < FA; ++i) { load_res(i, 0); load_res(i, 1); }
    glds_stage_rows<FA>(p, acc, 0, 0, wave_m, wave_n, frow, g, wbuf);
#pragma unroll
    for (int i = 0; i < FA; ++i) {
        const char* buf = wbuf + (i & 1) * 4096;
        if (i + 1 < FA) glds_stage_rows<FA>(p, acc, i + 1, 0, wave_m, wave_n, frow, g, wbuf + ((i + 1) & 1) * 4096);
#pragma unroll
        for (int ps = 0; ps < 2; ++ps) {
            const int R = 8 * ps + crow;
            float4_t v = glds_bounce_read(buf, R, 2 * cc), w = glds_bounce_read(buf, R, 2 * cc + 1);
            v += bias4; w += bias4b;
            add16(v, w, res[i % AHEAD][ps]);
            add16(v, w, res2[i % AHEAD][ps]);             // (zeros without a second residual)
            if (i + AHEAD < FA) load_res(i + AHEAD, ps);
            if constexpr (F16) amax = uc_amax(uc_amax(amax, uc_amax(uc_amax(fabsf(v.x), fabsf(v.y)), uc_amax(fabsf(v.z), fabsf(v.w)))),
                                              uc_amax(uc_amax(fabsf(w.x), fabsf(w.y)), uc_amax(fabsf(w.z), fabsf(w.w))));      // (NaN-propagating: common.h)
            const uint4_t pk = {glds_pack2<F16>(v.x, v.y), glds_pack2<F16>(v.z, v.w), glds_pack2<F16>(w.x, w.y), glds_pack2<F16>(w.z, w.w)};
            if (16 * i + 8 * ps < rows_left) {
                uint4_t* cq = reinterpret_cast<uint4_t*>(cbase + (2 * i + ps) * cstep + coff);
                if constexpr (NT) __builtin_nontemporal_store(pk, cq); else *cq = pk;
            }
        }
    }
    if constexpr (F16) {
        if (p.sat_flag && __any(!(amax <= UC_F16_MAX)) && lane == 0) atomicOr(p.sat_flag, 1);
    }
}

// LN: the folded-LayerNorm form — the accumulator holds x . W'^T of the RAW rows; row statistics and the column sums of W'
// turn it into LN(x) . W^T:  rstd[m] * (acc - mean[m] * colsum[n]) + bias[n].
template <int FA, int ACT, bool NT = false, bool LN = false, bool F16 = false>
__device__ __forceinline__ void glds_epilogue_bf16(glds_pe_t p, float4_t (&acc)[FA][4], int mode, int64_t wave_m,
                                                   int64_t wave_n, int lane, char* wbuf, const char* side = nullptr) {
    const int frow = lane & 15, g = lane >> 4;
    // Folded LayerNorm (LN): value = rstd[row] * (acc - mean[row] * colsum[col]) + bias[col], rows 16 i + frow, columns
    // 16 j + 4 g + r.  Lane l holds the statistics of row l of the wave tile (one coalesced load); a row block's pair comes
    // through ds_bpermute when the block is staged.  Applied where a value is consumed, never as an in-place pass over acc.
    // The LN form keeps its two column vectors (column sums, bias) of the wave's 64 columns in LDS behind the bounce
    // blocks and reads 16 bytes of each per fragment: held in registers (32 of them) next to the accumulators they spilled,
    // and a spill reload between global stores waits for every store before it (vmcnt counts stores, in order).
    float2 mine[FA / 4];
    float* colbuf = reinterpret_cast<float*>(wbuf + 4096);
    const float* biasbuf = colbuf + 64;
    if constexpr (LN) {
        if (side) {      // staged before the K-loop (side panel): no global load at the head of the epilogue
            colbuf = const_cast<float*>(reinterpret_cast<const float*>(side + GLDS_SIDE_COLSUM)) + (int)(wave_n & 255);
            biasbuf = reinterpret_cast<const float*>(side + GLDS_SIDE_BIAS) + (int)(wave_n & 255);
#pragma unroll
            for (int q = 0; q < FA / 4; ++q) mine[q] = reinterpret_cast<const float2*>(side + GLDS_SIDE_STATS)[(int)(wave_m & 255) + 64 * q + lane];
        } else {
            colbuf[lane] = p.ln_colsum[wave_n + lane];
            colbuf[64 + lane] = p.bias ? p.bias[wave_n + lane] : 0.f;
#pragma unroll
            for (int q = 0; q < FA / 4; ++q) mine[q] = glds_ln_row_stats<(FA > 4)>(p, min(wave_m + 64 * q + lane, p.M - 1));
        }
    }
    float st_mu = 0.f, st_rs = 1.f;
    auto row_stats = [&](int i) __attribute__((always_inline)) {
        if constexpr (LN) { st_mu = __shfl(mine[i / 4].x, 16 * (i & 3) + frow, 64); st_rs = __shfl(mine[i / 4].y, 16 * (i & 3) + frow, 64); }
    };
    float4_t b4[4];
    if constexpr (!LN) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            b4[j] = (float4_t){0.f, 0.f, 0.f, 0.f};
            if (p.bias) b4[j] = *reinterpret_cast<const float4_t*>(p.bias + wave_n + 16 * j + 4 * g);
        }
    }
    auto val4 = [&](int i, int j) __attribute__((always_inline)) -> float4_t {   // pre-activation values of fragment (i, j)
        if constexpr (LN) {
            const float4_t cs = *reinterpret_cast<const float4_t*>(colbuf + 16 * j + 4 * g);
            const float4_t bb = *reinterpret_cast<const float4_t*>(biasbuf + 16 * j + 4 * g);
            return glds_fma4(glds_fma4(glds_splat4(-st_mu), cs, acc[i][j]), glds_splat4(st_rs), bb);
        } else return acc[i][j] + b4[j];
    };
    // RoPE tiles: no loads inside the per-row-block code.  The table form (positions -> table address -> cos/sin, per row
    // block) was four dependent load chains per wave and cost 7 us per tile; here the positions of all row blocks are read up
    // front and the rotation angles go through the hardware sin/cos (argument in turns, v_fract first): 16 transcendentals
    // per row block per lane.  Channel 4g + r of a quarter has frequency F0 * base^(-(4g + r) / 16) (kernels.cu:36-81).
    unsigned pyx[FA];            // (y | x << 16) of row 16 i + frow: positions below 65536 (launcher-checked table size)
    float turn0 = 0.f;           // turns per unit position of channel 4g; channel 4g + r: turn0 * rope_ratio^r
    if (mode == 1) {
        turn0 = p.rope_turn0 * __builtin_amdgcn_exp2f((float)(4 * g) * p.rope_l2ratio);
#pragma unroll
        for (int i = 0; i < FA; ++i) {
            const int64_t m = min(wave_m + 16 * i + frow, p.M - 1);
            const longlong2 yx = (LN && side) ? *reinterpret_cast<const longlong2*>(side + GLDS_SIDE_POS + ((int)(wave_m & 255) + 16 * i + frow) * 16)
                                              : *reinterpret_cast<const longlong2*>(p.rope_pos + m * 2);
            pyx[i] = ((unsigned)min(max((int)yx.x, 0), 65535)) | ((unsigned)min(max((int)yx.y, 0), 65535) << 16);
        }
    }
    const int wr_off = frow * 128 + (((g & 1) ^ (frow >> 3)) << 3);       // + ((2j + (g>>1)) ^ (frow & 7)) << 4
    float amax = 0.f;            // fp16 stores: largest magnitude this lane packs (values beyond +-65504 saturate and raise p.sat_flag)
    auto stage = [&](int i, char* buf) {
        row_stats(i);
        if (mode == 1) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {      // fragment pair (2h, 2h+1) = channels d, d+16 of the y (h = 0) / x (h = 1) half
                const float pa = (float)(h ? (pyx[i] >> 16) : (pyx[i] & 0xffffu));
                const float4_t uu = val4(i, 2 * h), ww = val4(i, 2 * h + 1);
                float ou[4], ow[4];
                float turn = turn0;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float tfrac = __builtin_amdgcn_fractf(pa * turn);
                    turn *= p.rope_ratio;
                    const float cs = __builtin_amdgcn_cosf(tfrac), sn = __builtin_amdgcn_sinf(tfrac);
                    const float u = uu[r], w = ww[r];   // no activation with RoPE (launcher-checked)
                    ou[r] = __builtin_fmaf(u, cs, -(w * sn));
                    ow[r] = __builtin_fmaf(w, cs, u * sn);
                }
                *reinterpret_cast<uint2*>(buf + wr_off + (((4 * h + (g >> 1)) ^ (frow & 7)) << 4)) = (uint2){glds_pack2<F16>(ou[0], ou[1]), glds_pack2<F16>(ou[2], ou[3])};
                *reinterpret_cast<uint2*>(buf + wr_off + (((4 * h + 2 + (g >> 1)) ^ (frow & 7)) << 4)) = (uint2){glds_pack2<F16>(ow[0], ow[1]), glds_pack2<F16>(ow[2], ow[3])};
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float4_t v = glds_act4<ACT>(val4(i, j));
                if constexpr (F16) amax = uc_amax(uc_amax(amax, uc_amax(fabsf(v.x), fabsf(v.y))), uc_amax(fabsf(v.z), fabsf(v.w)));
                *reinterpret_cast<uint2*>(buf + wr_off + (((2 * j + (g >> 1)) ^ (frow & 7)) << 4)) = (uint2){glds_pack2<F16>(v.x, v.y), glds_pack2<F16>(v.z, v.w)};
            }
        }
    };
    const int crow = lane >> 3, pch = lane & 7;              // drain: row 8*ps + crow, physical chunk pch
    const int rows_left = (int)min((int64_t)(16 * FA), p.M - wave_m) - crow;
    char* cp = (char*)p.C + ((wave_m + crow) * p.ldc + wave_n) * 2;
    const int64_t cstep = 8 * p.ldc * 2;
    // Plain form: row block i + 1 is staged before block i is drained (its LDS writes overlap the global stores).  Folded-
    // LayerNorm form: 32 more registers (column sums, statistics) are live while staging, and a spill reload between global
    // stores waits for ALL of them (vmcnt counts stores, in order): the epilogue took 16 us instead of 6.  It stages all four
    // row blocks first — the wave's 8-KiB LDS block holds them as bf16 — and drains with no accumulator left alive.
    constexpr bool ALL_FIRST = false;   // (measured: staging all four row blocks first costs the LDS-write / store overlap: +2.9 us per tile)
    if constexpr (ALL_FIRST) {
#pragma unroll
        for (int i = 0; i < FA; ++i) stage(i, wbuf + i * 2048);
    } else {
        stage(0, wbuf);
    }
#pragma unroll
    for (int i = 0; i < FA; ++i) {
        const char* buf = ALL_FIRST ? wbuf + i * 2048 : wbuf + (i & 1) * 2048;
        if constexpr (!ALL_FIRST) {
            if (i + 1 < FA) stage(i + 1, wbuf + ((i + 1) & 1) * 2048);
        }
#pragma unroll
        for (int ps = 0; ps < 2; ++ps) {
            const int R = 8 * ps + crow;
            uint4 v = *reinterpret_cast<const uint4*>(buf + R * 128 + (pch << 4));
            if (ps) v = (uint4){v.z, v.w, v.x, v.y};         // rows 8..15 store their halves swapped
            if (16 * i + 8 * ps < rows_left) {
                if constexpr (NT) {
                    const uint4_t vv = (uint4_t){v.x, v.y, v.z, v.w};
                    __builtin_nontemporal_store(vv, reinterpret_cast<uint4_t*>(cp + ((pch ^ (R & 7)) << 4)));
                } else {
                    *reinterpret_cast<uint4*>(cp + ((pch ^ (R & 7)) << 4)) = v;
                }
            }
            cp += cstep;
        }
    }
    if constexpr (F16) {
        if (p.sat_flag && __any(!(amax <= UC_F16_MAX)) && lane == 0) atomicOr(p.sat_flag, 1);
    }
}

// Training forms of the bf16 store (mode 0 tiles, no residual): PRE also stores the value BEFORE the activation (fc1's
// pre-activation, saved for the backward), DACT multiplies the result by act'(u) of a saved pre-activation u laid out like C
// (the activation backward fused into the data-gradient GEMM).  Same bounce / whole-row stores as glds_epilogue_bf16; in the
// generic drain these two cost 60 % on top of the K = 1024 GEMMs that carry them (12 % of a training step).
template <int FA, int ACT, bool PRE, bool DACT>
__device__ __forceinline__ void glds_epilogue_bf16_train(glds_pe_t p, float4_t (&acc)[FA][4], int64_t wave_m, int64_t wave_n, int lane,
                                                         char* wbuf) {
    const int frow = lane & 15, g = lane >> 4;
    float4_t b4[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        b4[j] = (float4_t){0.f, 0.f, 0.f, 0.f};
        if (p.bias) b4[j] = *reinterpret_cast<const float4_t*>(p.bias + wave_n + 16 * j + 4 * g);
    }
    const int wr_off = frow * 128 + (((g & 1) ^ (frow >> 3)) << 3);
    auto stage = [&](int i, char* buf) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float4_t pre = acc[i][j] + b4[j];
            const int off = wr_off + (((2 * j + (g >> 1)) ^ (frow & 7)) << 4);
            if constexpr (PRE) *reinterpret_cast<uint2*>(buf + 4096 + off) = (uint2){pack_bf16x2(pre.x, pre.y), pack_bf16x2(pre.z, pre.w)};
            float4_t v = glds_act4<ACT>(pre);
            if constexpr (DACT) {
                // act'(u) multiplies the fp32 value, BEFORE the one rounding to bf16 (multiplying the rounded value in the drain and
                // rounding again put 6 % of the elements more than half an ulp off: tests/test_gemm_routes_gpu.py); rows past M read row M - 1
                const int64_t m = min(wave_m + 16 * i + frow, p.M - 1);
                const uint2 u = *reinterpret_cast<const uint2*>((const char*)p.dact_u + (m * p.ldc + wave_n + 16 * j + 4 * g) * 2);
                v.x *= glds_dact(__uint_as_float(u.x << 16), p.dact_act);
                v.y *= glds_dact(__uint_as_float(u.x & 0xffff0000u), p.dact_act);
                v.z *= glds_dact(__uint_as_float(u.y << 16), p.dact_act);
                v.w *= glds_dact(__uint_as_float(u.y & 0xffff0000u), p.dact_act);
            }
            *reinterpret_cast<uint2*>(buf + off) = (uint2){pack_bf16x2(v.x, v.y), pack_bf16x2(v.z, v.w)};
        }
    };
    const int crow = lane >> 3, pch = lane & 7;
    const int rows_left = (int)min((int64_t)(16 * FA), p.M - wave_m) - crow;
    const int64_t row0 = ((wave_m + crow) * p.ldc + wave_n) * 2;           // byte offset of (row, column block) in C / preact / dact_u
    const int64_t cstep = 8 * p.ldc * 2;
    stage(0, wbuf);
#pragma unroll
    for (int i = 0; i < FA; ++i) {
        const char* buf = wbuf + (i & 1) * 2048;
        if (i + 1 < FA) stage(i + 1, wbuf + ((i + 1) & 1) * 2048);
#pragma unroll
        for (int ps = 0; ps < 2; ++ps) {
            const int R = 8 * ps + crow;
            const int64_t off = row0 + (2 * i + ps) * cstep + ((pch ^ (R & 7)) << 4);
            uint4 v = *reinterpret_cast<const uint4*>(buf + R * 128 + (pch << 4));
            if (ps) v = (uint4){v.z, v.w, v.x, v.y};         // rows 8..15 keep their halves swapped in the bounce block
            if (16 * i + 8 * ps < rows_left) {
                *reinterpret_cast<uint4*>((char*)p.C + off) = v;
                if constexpr (PRE) {
                    uint4 w = *reinterpret_cast<const uint4*>(buf + 4096 + R * 128 + (pch << 4));
                    if (ps) w = (uint4){w.z, w.w, w.x, w.y};
                    *reinterpret_cast<uint4*>((char*)p.preact + off) = w;
                }
            }
        }
    }
}

// 4 values of row m, columns nb..nb+3 of a [*, ld] matrix of dtype dt: vector access when `full`, else per element inside N
__device__ __forceinline__ float4_t glds_load4(const void* base, int dt, int64_t idx, bool full, int64_t nb, int64_t N) {
    float4_t v = (float4_t){0.f, 0.f, 0.f, 0.f};
    if (full) {
        if (dt == UC_F32) v = *reinterpret_cast<const float4_t*>((const float*)base + idx);
        else if (dt == UC_F16) v = glds_unpack_f16x4(*reinterpret_cast<const uint2*>((const bf16_t*)base + idx));
        else {
            const uint2 q = *reinterpret_cast<const uint2*>((const bf16_t*)base + idx);
            v = (float4_t){__uint_as_float(q.x << 16), __uint_as_float(q.x & 0xffff0000u), __uint_as_float(q.y << 16), __uint_as_float(q.y & 0xffff0000u)};
        }
    } else {
        for (int r = 0; r < 4; ++r)
            if (nb + r < N) v[r] = dt == UC_F32 ? ((const float*)base)[idx + r] : (dt == UC_F16 ? f16_to_f32(((const bf16_t*)base)[idx + r]) : bf16_to_f32(((const bf16_t*)base)[idx + r]));
    }
    return v;
}
__device__ __forceinline__ void glds_store4(void* base, int dt, int64_t idx, bool full, int64_t nb, int64_t N, float4_t v) {
    if (full) {
        if (dt == UC_F32) *reinterpret_cast<float4_t*>((float*)base + idx) = v;
        else if (dt == UC_F16) *reinterpret_cast<uint2*>((bf16_t*)base + idx) = (uint2){glds_pack2<true>(v.x, v.y), glds_pack2<true>(v.z, v.w)};
        else *reinterpret_cast<uint2*>((bf16_t*)base + idx) = (uint2){pack_bf16x2(v.x, v.y), pack_bf16x2(v.z, v.w)};
    } else {
        for (int r = 0; r < 4; ++r) {
            if (nb + r >= N) continue;
            if (dt == UC_F32) ((float*)base)[idx + r] = v[r];
            else if (dt == UC_F16) ((bf16_t*)base)[idx + r] = f32_to_f16(v[r]);
            else ((bf16_t*)base)[idx + r] = f32_to_bf16(v[r]);
        }
    }
}

template <int FA>
__device__ __forceinline__ void glds_epilogue_generic(glds_pe_t p, float4_t (&acc)[FA][4], int mode, int64_t wave_m,
                                                      int64_t wave_n, int lane, int ksplit, char* wbuf) {
    const int frow = lane & 15, g = lane >> 4;
    const int crow = lane >> 4, cchunk = lane & 15;
    const int64_t nb = wave_n + 4 * cchunk;
    const bool full = p.vec_ok && nb + 3 < p.N;
    float4_t bias4 = (float4_t){0.f, 0.f, 0.f, 0.f};
    if (mode != 1 && p.bias && p.split_k <= 1) bias4 = glds_load4(p.bias, UC_F32, nb, full, nb, p.N);
    float* slab = (float*)p.C + (int64_t)ksplit * p.M * p.ldc;
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < FA; ++i) {
        char* buf = wbuf + (i & 1) * 4096;
        glds_stage_rows<FA>(p, acc, i, mode, wave_m, wave_n, frow, g, buf);
#pragma unroll 1
        for (int ps = 0; ps < 4; ++ps) {
            const int R = 4 * ps + crow;
            float4_t v = glds_bounce_read(buf, R, cchunk);
            const int64_t m = wave_m + 16 * i + R;
            if (m >= p.M || nb >= p.N) continue;
            const int64_t ci = m * p.ldc + nb;
            if (p.split_k > 1) { glds_store4(slab, UC_F32, ci, full, nb, p.N, v); continue; }
            if (mode != 1) {
                v += bias4;
                if (p.preact) glds_store4(p.preact, p.out_dtype, ci, full, nb, p.N, v);
                if (p.act == UC_ACT_GELU_ERF) { for (int r = 0; r < 4; ++r) v[r] = glds_gelu(v[r]); }
                else if (p.act == UC_ACT_RELU) { for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f); }
            }
            if (p.residual) {
                v += glds_load4(p.residual, p.res_dtype, m * p.ldr + nb, full, nb, p.N);
                if (p.residual2) v += glds_load4(p.residual2, p.res_dtype, m * p.ldr + nb, full, nb, p.N);
            }
            if (p.dact_u) {   // fused activation backward: out = v * act'(u)
                const float4_t u = glds_load4(p.dact_u, UC_BF16, ci, full, nb, p.N);
                if (p.dact_act == UC_ACT_RELU) { for (int r = 0; r < 4; ++r) v[r] = u[r] > 0.f ? v[r] : 0.f; }
                else { for (int r = 0; r < 4; ++r) v[r] *= glds_dact(u[r], UC_ACT_GELU_ERF); }
            }
            amax = uc_amax(uc_amax(amax, uc_amax(fabsf(v.x), fabsf(v.y))), uc_amax(fabsf(v.z), fabsf(v.w)));
            glds_store4(p.C, p.out_dtype, ci, full, nb, p.N, v);
        }
    }
    // fp16 outputs saturate at +-65504 (glds_store4): tell the caller when they did
    if (p.out_dtype == UC_F16 && p.sat_flag && __any(!(amax <= UC_F16_MAX)) && lane == 0) atomicOr(p.sat_flag, 1);
}

// Fused narrow tail of a 128-wide tile (two wave columns of 64): out4[m][o] = tail_b[o] + sum_n act(acc[m][n] + bias[n]) * tail_w[o][n].
// The DPT regressor's conv3x3 -> ReLU -> Conv2d(128 -> 4, 1x1): the 128-channel map is never stored.  Per wave: its 64 columns of
// tail_w (as float4 over the four outputs) and of the bias sit in its LDS block; a lane multiplies its 16 values of a row by
// them, the four lanes that share a row (lane bits 4, 5) add up through two xor-shuffles, the two wave columns meet through
// LDS, and the left wave column stores 64 rows x 16 bytes — one contiguous KiB.
template <int FA, int ACT>
__device__ __forceinline__ void glds_epilogue_tail4(glds_pe_t p, float4_t (&acc)[FA][4], int64_t wave_m, int64_t wave_n, int lane,
                                                    int wave, char* smem) {
    static_assert(FA == 4, "the fused tail is written for 64-row wave tiles");
    const int frow = lane & 15, g = lane >> 4;
    char* wbuf = smem + wave * 8192;
    float4_t* wl = reinterpret_cast<float4_t*>(wbuf);              // [64 columns] x (o = 0..3)
    float* bl = reinterpret_cast<float*>(wbuf + 1024);            // [64] bias
    float4_t* xl = reinterpret_cast<float4_t*>(wbuf + 2048);       // [64 rows] partial sums of this wave column
    {
        const int64_t n = wave_n + lane;
        wl[lane] = (float4_t){p.tail_w[n], p.tail_w[p.N + n], p.tail_w[2 * p.N + n], p.tail_w[3 * p.N + n]};
        bl[lane] = p.bias ? p.bias[n] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < FA; ++i) {
        float4_t s = (float4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float4_t b4 = *reinterpret_cast<const float4_t*>(bl + 16 * j + 4 * g);
            const float4_t v = glds_act4<ACT>(acc[i][j] + b4);
#pragma unroll
            for (int r = 0; r < 4; ++r) s += v[r] * wl[16 * j + 4 * g + r];
        }
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            s[o] += __shfl_xor(s[o], 16, 64);
            s[o] += __shfl_xor(s[o], 32, 64);
        }
        if (g == 0) xl[16 * i + frow] = s;
    }
    __syncthreads();                                             // both wave columns of every row block have written their partials
    if ((wave & 1) == 0) {                                       // wave = 2 * wave_row + wave_column in every 128-wide tile variant
        const float4_t* other = reinterpret_cast<const float4_t*>(smem + (wave + 1) * 8192 + 2048);
        float4_t o = xl[lane] + other[lane];
        if (p.tail_b) o += (float4_t){p.tail_b[0], p.tail_b[1], p.tail_b[2], p.tail_b[3]};
        if (wave_m + lane < p.M) *reinterpret_cast<float4_t*>(p.tail_out + (wave_m + lane) * 4) = o;
    }
}

// Epilogue dispatch shared by the 16-wave and the 8-wave kernels: picks the drain of this wave's 64-column block from the family
// compiled into the instantiation (EPI) and the wave's mode (0 plain, 1 RoPE, 2 packed-VT).
template <int FA, int A_MODE, int EPI, bool F16 = false>
__device__ __forceinline__ void glds_epilogue_dispatch(glds_pe_t pe, float4_t (&acc)[FA][4], int mode, int64_t wave_m, int64_t wave_n,
                                                       int tid, int wave, int ksplit, char* smem, const char* side = nullptr) {
    static_assert(!F16 || EPI == GLDS_EPI_ALL || EPI == GLDS_EPI_RES16, "the fp16 operand form exists in the EPI_ALL and RES16 families only");
    constexpr int OUT16 = F16 ? UC_F16 : UC_BF16;        // the 16-bit storage dtype of this instantiation
    if (wave_n >= pe.N) return;
    {
        // a fresh definition of the lane id: keeps the compiler from hoisting the epilogue's per-lane address math above
        // the K-loop, where it spilled loop-carried registers of the 128-VGPR kernels
        int lane = tid & 63;
        asm volatile("" : "+v"(lane));
        char* wbuf = smem + wave * 8192;
        // (the launcher routes a descriptor to the BF16 / F32 family only when every tile of it takes that family's epilogue)
        const bool plain = pe.vec_ok && wave_n + 64 <= pe.N && pe.split_k <= 1 && !pe.preact && !pe.dact_u && !UC_DBG(pe, 16);
        auto bf16_family = [&]() __attribute__((always_inline)) {
            const bool nt = pe.nt_out & (mode == 1 ? 4 : 2);
            if (!F16 && A_MODE == UC_A_DENSE && (pe.ln_stats || pe.ln_partial)) {   // folded LayerNorm
                if constexpr (A_MODE == UC_A_DENSE && !F16) {
                    if (nt) {
                        if (pe.act == UC_ACT_GELU_ERF) glds_epilogue_bf16<FA, UC_ACT_GELU_ERF, true, true>(pe, acc, mode, wave_m, wave_n, lane, wbuf, side);
                        else glds_epilogue_bf16<FA, UC_ACT_NONE, true, true>(pe, acc, mode, wave_m, wave_n, lane, wbuf, side);
                    } else {
                        if (pe.act == UC_ACT_GELU_ERF) glds_epilogue_bf16<FA, UC_ACT_GELU_ERF, false, true>(pe, acc, mode, wave_m, wave_n, lane, wbuf, side);
                        else glds_epilogue_bf16<FA, UC_ACT_NONE, false, true>(pe, acc, mode, wave_m, wave_n, lane, wbuf, side);
                    }
                }
            } else if (nt) {
                if (pe.act == UC_ACT_GELU_ERF) glds_epilogue_bf16<FA, UC_ACT_GELU_ERF, true, false, F16>(pe, acc, mode, wave_m, wave_n, lane, wbuf);
                else if (pe.act == UC_ACT_RELU) glds_epilogue_bf16<FA, UC_ACT_RELU, true, false, F16>(pe, acc, mode, wave_m, wave_n, lane, wbuf);
                else glds_epilogue_bf16<FA, UC_ACT_NONE, true, false, F16>(pe, acc, mode, wave_m, wave_n, lane, wbuf);
            } else {
                if (pe.act == UC_ACT_GELU_ERF) glds_epilogue_bf16<FA, UC_ACT_GELU_ERF, false, false, F16>(pe, acc, mode, wave_m, wave_n, lane, wbuf);
                else if (pe.act == UC_ACT_RELU) glds_epilogue_bf16<FA, UC_ACT_RELU, false, false, F16>(pe, acc, mode, wave_m, wave_n, lane, wbuf);
                else glds_epilogue_bf16<FA, UC_ACT_NONE, false, false, F16>(pe, acc, mode, wave_m, wave_n, lane, wbuf);
            }
        };
        auto f32_family = [&]() __attribute__((always_inline)) {
            if (pe.nt_out & 1) glds_epilogue_resid<FA, true>(pe, acc, mode, wave_m, wave_n, lane, wbuf);
            else glds_epilogue_resid<FA, false>(pe, acc, mode, wave_m, wave_n, lane, wbuf);
        };
        if constexpr (EPI == GLDS_EPI_BF16) {
            if (mode == 2) {
                // (a 128-row wave tile drains as two 64-row halves: the packed-VT fast path is one aligned 64-token group)
                if constexpr (FA == 4) {
                    if (A_MODE == UC_A_DENSE && (pe.ln_stats || pe.ln_partial)) glds_epilogue_vt<4, A_MODE == UC_A_DENSE>(pe, acc, wave_m, wave_n, lane, wbuf);
                    else glds_epilogue_vt<4>(pe, acc, wave_m, wave_n, lane, wbuf);
                } else {
#pragma unroll
                    for (int h = 0; h < FA / 4; ++h) {
                        float4_t half[4][4];
#pragma unroll
                        for (int i = 0; i < 4; ++i)
#pragma unroll
                            for (int j = 0; j < 4; ++j) half[i][j] = acc[4 * h + i][j];
                        if (A_MODE == UC_A_DENSE && (pe.ln_stats || pe.ln_partial)) glds_epilogue_vt<4, A_MODE == UC_A_DENSE, true>(pe, half, wave_m + 64 * h, wave_n, lane, wbuf, side);
                        else glds_epilogue_vt<4>(pe, half, wave_m + 64 * h, wave_n, lane, wbuf);
                    }
                }
            } else bf16_family();
        } else if constexpr (EPI == GLDS_EPI_F32) {
            f32_family();
        } else if constexpr (EPI == GLDS_EPI_RES16) {       // convolution with 16-bit residual(s) laid out like its 16-bit output (launcher: glds_res16_ok)
            if (pe.nt_out & 2) glds_epilogue_res16<FA, true, F16>(pe, acc, wave_m, wave_n, lane, wbuf);
            else glds_epilogue_res16<FA, false, F16>(pe, acc, wave_m, wave_n, lane, wbuf);
        } else if constexpr (EPI == GLDS_EPI_BS) {          // bf16 residual stream: bf16 output + bf16 residual(s) + row statistics
            if (pe.nt_out & 1) glds_epilogue_bs<FA, true>(pe, acc, mode, wave_m, wave_n, lane, wbuf);
            else glds_epilogue_bs<FA, false>(pe, acc, mode, wave_m, wave_n, lane, wbuf);
        } else {
            if constexpr (A_MODE != UC_A_DENSE && FA == 4) {
                if (pe.tail_out) {      // (launcher: N == 128 on a 128-wide tile, every wave of the workgroup arrives here)
                    if (pe.act == UC_ACT_RELU) glds_epilogue_tail4<FA, UC_ACT_RELU>(pe, acc, wave_m, wave_n, lane, wave, smem);
                    else if (pe.act == UC_ACT_GELU_ERF) glds_epilogue_tail4<FA, UC_ACT_GELU_ERF>(pe, acc, wave_m, wave_n, lane, wave, smem);
                    else glds_epilogue_tail4<FA, UC_ACT_NONE>(pe, acc, wave_m, wave_n, lane, wave, smem);
                    return;
                }
            } else if constexpr (A_MODE != UC_A_DENSE && FA == 8) {
                if (pe.tail_out) {      // a 128-row wave tile (eight-wave conv kernel, 4 x 2 waves) drains as two 64-row halves
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        float4_t half[4][4];
#pragma unroll
                        for (int i = 0; i < 4; ++i)
#pragma unroll
                            for (int j = 0; j < 4; ++j) half[i][j] = acc[4 * h + i][j];
                        if (h) __syncthreads();     // the left wave columns have read the first half's partial sums
                        if (pe.act == UC_ACT_RELU) glds_epilogue_tail4<4, UC_ACT_RELU>(pe, half, wave_m + 64 * h, wave_n, lane, wave, smem);
                        else if (pe.act == UC_ACT_GELU_ERF) glds_epilogue_tail4<4, UC_ACT_GELU_ERF>(pe, half, wave_m + 64 * h, wave_n, lane, wave, smem);
                        else glds_epilogue_tail4<4, UC_ACT_NONE>(pe, half, wave_m + 64 * h, wave_n, lane, wave, smem);
                    }
                    return;
                }
            }
            if (!F16 && mode == 2) {
                if constexpr (F16) { }
                else if constexpr (FA == 4) glds_epilogue_vt<4>(pe, acc, wave_m, wave_n, lane, wbuf);
                else {
#pragma unroll
                    for (int h = 0; h < FA / 4; ++h) {
                        float4_t half[4][4];
#pragma unroll
                        for (int i = 0; i < 4; ++i)
#pragma unroll
                            for (int j = 0; j < 4; ++j) half[i][j] = acc[4 * h + i][j];
                        glds_epilogue_vt<4>(pe, half, wave_m + 64 * h, wave_n, lane, wbuf);
                    }
                }
            } else if (plain && pe.out_dtype == OUT16 && !pe.residual) bf16_family();

            else if (!F16 && mode == 0 && pe.vec_ok && wave_n + 64 <= pe.N && pe.split_k <= 1 && pe.out_dtype == UC_BF16 && !pe.residual &&
                     !UC_DBG(pe, 16) && !pe.ln_stats && !pe.ln_partial && (pe.preact != nullptr) != (pe.dact_u != nullptr)) {
                // training: fc1 with its pre-activation copy / a data-gradient GEMM with the activation backward fused
                if (pe.preact) {
                    if (pe.act == UC_ACT_GELU_ERF) glds_epilogue_bf16_train<FA, UC_ACT_GELU_ERF, true, false>(pe, acc, wave_m, wave_n, lane, wbuf);
                    else if (pe.act == UC_ACT_RELU) glds_epilogue_bf16_train<FA, UC_ACT_RELU, true, false>(pe, acc, wave_m, wave_n, lane, wbuf);
                    else glds_epilogue_bf16_train<FA, UC_ACT_NONE, true, false>(pe, acc, wave_m, wave_n, lane, wbuf);
                } else if (pe.act == UC_ACT_NONE) glds_epilogue_bf16_train<FA, UC_ACT_NONE, false, true>(pe, acc, wave_m, wave_n, lane, wbuf);
                else glds_epilogue_generic<FA>(pe, acc, mode, wave_m, wave_n, lane, ksplit, wbuf);
            }
            else if (plain && pe.out_dtype == UC_F32 && (!pe.residual || pe.res_dtype == UC_F32) && pe.act == UC_ACT_NONE) f32_family();
            else glds_epilogue_generic<FA>(pe, acc, mode, wave_m, wave_n, lane, ksplit, wbuf);
        }
    }
}
