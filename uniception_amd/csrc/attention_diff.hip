// Differential attention forward (one launch) and the backward of its combine step.
//   A1 = softmax(scale Q1 K1^T) V, A2 = softmax(scale Q2 K2^T) V, a = A1 - lambda A2, O = RMSNorm(a; w, eps) * out_scale
// (reference: models/utils/transformer_blocks.py:686-945, DiffAttention / DiffCrossAttention; arXiv 2410.05258).
//
// bf16 kernel (diff_attn_bf16_kernel): the register-staged 128-query kernel of attention.hip (attn_bf16_body) with two score
// products per key tile.  256 threads = 4 waves x 32 queries; per 64-key tile ONE 8 KB LDS tile holds K1 | K2 (row = key, bytes
// 0..63 the 32 channels of head h, bytes 64..127 those of head H + h) and one 8 KB tile the packed V^T [64 channels][64 positions];
// both are double buffered (32 KB LDS).  S1^T = K1 Q1^T and S2^T = K2 Q2^T are two 32x32x16 MFMA steps per 32-key block each, the
// two online softmaxes keep their own (max, sum), and every V^T fragment read from LDS feeds two MFMAs (O1^T and O2^T).  A lane
// pair (lane, lane ^ 32) holds the 64 channels of one query in both accumulators, so the combine + RMSNorm epilogue needs one
// cross-lane add.  Registers: 4 x 16 accumulators + 2 x 32 scores + 2 x 16 packed probabilities + 16 Q fragment + 16 staging.
// fp32 kernel (diff_attn_f32_kernel): one thread per query in the style of attn_f32_kernel, 32-key tiles of K1, K2 and V in LDS.
#include "attention_tile.h"

struct DiffParams {
    const void* Q;
    const void* K;
    const void* V;
    void* O;
    void* A1;
    void* A2;
    float* lse1;
    float* lse2;
    const float* w;
    int B, H, Nq, Nk, Dqk;
    int64_t q_sb, q_sn, q_sh, k_sb, k_sn, k_sh, v_sb, v_sn, v_sh, o_sb, o_sn, o_sh;
    int npad;
    float scale, lambda, eps, out_scale;
};

__global__ __launch_bounds__(256) void diff_attn_bf16_kernel(DiffParams p) {
    __shared__ __attribute__((aligned(16))) char smem[4 * ATT_TILE_BYTES];   // 2 stages x (K1|K2 tile + VT tile)
    const int b = blockIdx.z, h = blockIdx.y;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int hi = lane >> 5;
    const int l31 = lane & 31;
    const int q0 = (int)blockIdx.x * 128 + wave * 32;

    const bf16_t* Qb = (const bf16_t*)p.Q + (int64_t)b * p.q_sb;
    const bf16_t* Kb1 = (const bf16_t*)p.K + (int64_t)b * p.k_sb + (int64_t)h * p.k_sh;
    const bf16_t* Kb2 = (const bf16_t*)p.K + (int64_t)b * p.k_sb + (int64_t)(p.H + h) * p.k_sh;
    const bf16_t* VTb = (const bf16_t*)p.V + ((int64_t)b * p.H + h) * 64 * (int64_t)p.npad;

    // Q^T fragments (B operand): lane (q = l31, hi) holds Q1[q][16 s + 8 hi .. + 7] in qf[s], Q2[q][..] in qf[2 + s], s = 0, 1
    bf16x8_t qf[4];
    {
        int q = q0 + l31;
        if (q >= p.Nq) q = p.Nq - 1;   // clamp; rows beyond Nq are never stored
        const bf16_t* q1 = Qb + (int64_t)q * p.q_sn + (int64_t)h * p.q_sh + hi * 8;
        const bf16_t* q2 = Qb + (int64_t)q * p.q_sn + (int64_t)(p.H + h) * p.q_sh + hi * 8;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            qf[s] = *reinterpret_cast<const bf16x8_t*>(q1 + 16 * s);
            qf[2 + s] = *reinterpret_cast<const bf16x8_t*>(q2 + 16 * s);
        }
    }

    // staging: 512 16-byte chunks per tile, 2 per thread (rows sr and sr + 32, chunk column cc)
    const int cc = tid & 7;
    const int sr = tid >> 3;
    const bf16_t* Ksrc = (cc < 4 ? Kb1 : Kb2) + (cc & 3) * 8;
    uint4 rk0, rk1, rv0, rv1;
    auto load_k = [&](int k0, int row) -> uint4 {
        int key = k0 + row;
        if (key >= p.Nk) key = p.Nk - 1;   // clamped keys are masked in the softmax
        return *reinterpret_cast<const uint4*>(Ksrc + (int64_t)key * p.k_sn);
    };
    auto load_v = [&](int k0, int row) -> uint4 { return att_load_vt_chunk(VTb, row, p.npad, k0, cc, p.Nk); };
#define DIFF_STAGE_LOAD(k0_)                \
    do {                                    \
        rk0 = load_k((k0_), sr);            \
        rk1 = load_k((k0_), sr + 32);       \
        rv0 = load_v((k0_), sr);            \
        rv1 = load_v((k0_), sr + 32);       \
    } while (0)
    const int w_off = tile_swz(sr, cc);   // rows r and r + 32 share the swizzle key
#define DIFF_STAGE_WRITE(buf_)                                                 \
    do {                                                                       \
        char* sk_ = smem + (buf_) * 2 * ATT_TILE_BYTES + w_off;                   \
        *reinterpret_cast<uint4*>(sk_) = rk0;                                  \
        *reinterpret_cast<uint4*>(sk_ + 32 * 128) = rk1;                       \
        *reinterpret_cast<uint4*>(sk_ + ATT_TILE_BYTES) = rv0;                    \
        *reinterpret_cast<uint4*>(sk_ + ATT_TILE_BYTES + 32 * 128) = rv1;         \
    } while (0)
    int r_off[4];   // K tile: st 0, 1 = K1, st 2, 3 = K2; VT tile: 16-key slab st
    att_frag_offsets(r_off, l31, hi);

    float16_t o1[2], o2[2];   // O^T accumulators: channel d = att_frag_row(db, r, hi), query l31
    o1[0] = o1[1] = o2[0] = o2[1] = (float16_t)(0.f);
    float m1 = ATT_MASKED, m2 = ATT_MASKED, l1 = 0.f, l2 = 0.f;
    const float c = p.scale * ATT_LOG2E;

    const int nt = (p.Nk + ATT_KV_TILE - 1) / ATT_KV_TILE;
    DIFF_STAGE_LOAD(0);
    DIFF_STAGE_WRITE(0);
    __syncthreads();

    for (int t = 0; t < nt; ++t) {
        const int buf = t & 1;
        const int k0 = t * ATT_KV_TILE;
        if (t + 1 < nt) DIFF_STAGE_LOAD(k0 + ATT_KV_TILE);
        const char* sk = smem + buf * 2 * ATT_TILE_BYTES;
        const char* sv = sk + ATT_TILE_BYTES;

        float16_t s1[2], s2[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            s1[kb] = (float16_t)(0.f);
            s2[kb] = (float16_t)(0.f);
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                const bf16x8_t k1f = *reinterpret_cast<const bf16x8_t*>(sk + r_off[st] + kb * (32 * 128));
                const bf16x8_t k2f = *reinterpret_cast<const bf16x8_t*>(sk + r_off[2 + st] + kb * (32 * 128));
                s1[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(k1f, qf[st], s1[kb], 0, 0, 0);
                s2[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(k2f, qf[2 + st], s2[kb], 0, 0, 0);
            }
        }
        if (k0 + ATT_KV_TILE > p.Nk) {
            att_mask_tail(s1, k0, p.Nk, hi);
            att_mask_tail(s2, k0, p.Nk, hi);
        }
        AttProbsBf16 pr1, pr2;
        att_softmax_step(s1, m1, l1, o1, c, pr1);
        att_softmax_step(s2, m2, l2, o2, c, pr2);

        // O1^T += V^T P1^T, O2^T += V^T P2^T: every V^T fragment is read once and feeds both
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const bf16x8_t vf = *reinterpret_cast<const bf16x8_t*>(sv + r_off[g] + db * (32 * 128));
                o1[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pr1.pf[g], o1[db], 0, 0, 0);
                o2[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pr2.pf[g], o2[db], 0, 0, 0);
            }

        if (t + 1 < nt) DIFF_STAGE_WRITE(buf ^ 1);
        __syncthreads();
    }
#undef DIFF_STAGE_LOAD
#undef DIFF_STAGE_WRITE

    // ---- epilogue: a = O1 / l1 - lambda O2 / l2, y = a rsqrt(mean a^2 + eps) w out_scale, all in fp32 ----
    const float l1t = l1 + __shfl_xor(l1, 32, 64);
    const float l2t = l2 + __shfl_xor(l2, 32, 64);
    const float inv1 = 1.0f / l1t, inv2 = 1.0f / l2t;
    float ss = 0.f;
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            o1[db][r] *= inv1;
            o2[db][r] *= inv2;
            const float a = o1[db][r] - p.lambda * o2[db][r];
            ss = fmaf(a, a, ss);
        }
    ss += __shfl_xor(ss, 32, 64);
    const float rr = 1.0f / sqrtf(ss * (1.0f / 64.0f) + p.eps);
    const int q = q0 + l31;
    if (q >= p.Nq) return;
    const int64_t bh = (int64_t)b * p.H + h;
    if (p.lse1 && hi == 0) {
        p.lse1[bh * p.Nq + q] = m1 * p.scale + logf(l1t);
        p.lse2[bh * p.Nq + q] = m2 * p.scale + logf(l2t);
    }
    bf16_t* op = (bf16_t*)p.O + (int64_t)b * p.o_sb + (int64_t)q * p.o_sn + (int64_t)h * p.o_sh;
    const int64_t arow = (((int64_t)b * p.Nq + q) * p.H + h) * 64;
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const int d = db * 32 + 8 * g4 + 4 * hi;
            const float4 wv = *reinterpret_cast<const float4*>(p.w + d);
            const float wj[4] = {wv.x, wv.y, wv.z, wv.w};
            float y[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float a = o1[db][g4 * 4 + j] - p.lambda * o2[db][g4 * 4 + j];
                y[j] = ((a * rr) * wj[j]) * p.out_scale;
            }
            uint2 pk;
            pk.x = pack_bf16x2(y[0], y[1]);
            pk.y = pack_bf16x2(y[2], y[3]);
            *reinterpret_cast<uint2*>(op + d) = pk;
            if (p.A1) {
                pk.x = pack_bf16x2(o1[db][g4 * 4 + 0], o1[db][g4 * 4 + 1]);
                pk.y = pack_bf16x2(o1[db][g4 * 4 + 2], o1[db][g4 * 4 + 3]);
                *reinterpret_cast<uint2*>((bf16_t*)p.A1 + arow + d) = pk;
                pk.x = pack_bf16x2(o2[db][g4 * 4 + 0], o2[db][g4 * 4 + 1]);
                pk.y = pack_bf16x2(o2[db][g4 * 4 + 2], o2[db][g4 * 4 + 3]);
                *reinterpret_cast<uint2*>((bf16_t*)p.A2 + arow + d) = pk;
            }
        }
}

// ---------------------------------------------------------------------------------------
// fp32 verification kernel: one thread per query, 32-key tiles of K1, K2 and V in LDS (broadcast reads); Dqk <= 32, V has 2 Dqk <= 64
// ---------------------------------------------------------------------------------------
#define DF32_KT 32

__device__ __forceinline__ void diff_f32_softmax_step(const float (&s)[DF32_KT], const float mt, float& m_run, float& l_run, float (&acc)[64],
                                                      const float (*Vs)[64], const int k0, const int Nk) {
    const float m_new = fmaxf(m_run, mt);
    const float alpha = (m_run == -INFINITY) ? 0.f : expf(m_run - m_new);
    l_run *= alpha;
#pragma unroll
    for (int d = 0; d < 64; ++d) acc[d] *= alpha;
#pragma unroll
    for (int kk = 0; kk < DF32_KT; ++kk) {
        const float pw = (k0 + kk < Nk) ? expf(s[kk] - m_new) : 0.f;
        l_run += pw;
#pragma unroll
        for (int d = 0; d < 64; ++d) acc[d] = fmaf(pw, Vs[kk][d], acc[d]);
    }
    m_run = m_new;
}

__global__ __launch_bounds__(128) void diff_attn_f32_kernel(DiffParams p) {
    __shared__ float K1s[DF32_KT][32];
    __shared__ float K2s[DF32_KT][32];
    __shared__ float Vs[DF32_KT][64];
    const int b = blockIdx.z, h = blockIdx.y;
    const int q = blockIdx.x * 128 + threadIdx.x;
    const int D = p.Dqk, DV = 2 * p.Dqk;
    const float* Q1 = (const float*)p.Q + (int64_t)b * p.q_sb + (int64_t)h * p.q_sh;
    const float* Q2 = (const float*)p.Q + (int64_t)b * p.q_sb + (int64_t)(p.H + h) * p.q_sh;
    const float* K1 = (const float*)p.K + (int64_t)b * p.k_sb + (int64_t)h * p.k_sh;
    const float* K2 = (const float*)p.K + (int64_t)b * p.k_sb + (int64_t)(p.H + h) * p.k_sh;
    const float* Vb = (const float*)p.V + (int64_t)b * p.v_sb + (int64_t)h * p.v_sh;
    const bool active = q < p.Nq;
    float q1[32], q2[32], a1[64], a2[64];
#pragma unroll
    for (int d = 0; d < 32; ++d) {
        q1[d] = (active && d < D) ? Q1[(int64_t)q * p.q_sn + d] : 0.f;
        q2[d] = (active && d < D) ? Q2[(int64_t)q * p.q_sn + d] : 0.f;
    }
#pragma unroll
    for (int d = 0; d < 64; ++d) a1[d] = a2[d] = 0.f;
    float m1 = -INFINITY, m2 = -INFINITY, l1 = 0.f, l2 = 0.f;
    for (int k0 = 0; k0 < p.Nk; k0 += DF32_KT) {
        __syncthreads();
        for (int idx = threadIdx.x; idx < DF32_KT * 32; idx += blockDim.x) {
            const int kk = idx >> 5, d = idx & 31;
            const bool ok = (k0 + kk < p.Nk) && d < D;
            K1s[kk][d] = ok ? K1[(int64_t)(k0 + kk) * p.k_sn + d] : 0.f;
            K2s[kk][d] = ok ? K2[(int64_t)(k0 + kk) * p.k_sn + d] : 0.f;
        }
        for (int idx = threadIdx.x; idx < DF32_KT * 64; idx += blockDim.x) {
            const int kk = idx >> 6, d = idx & 63;
            Vs[kk][d] = ((k0 + kk < p.Nk) && d < DV) ? Vb[(int64_t)(k0 + kk) * p.v_sn + d] : 0.f;
        }
        __syncthreads();
        float s[DF32_KT];
        float mt = -INFINITY;
#pragma unroll
        for (int kk = 0; kk < DF32_KT; ++kk) {
            float a = 0.f;
#pragma unroll
            for (int d = 0; d < 32; ++d) a = fmaf(q1[d], K1s[kk][d], a);
            a *= p.scale;
            s[kk] = (k0 + kk < p.Nk) ? a : -INFINITY;
            mt = fmaxf(mt, s[kk]);
        }
        diff_f32_softmax_step(s, mt, m1, l1, a1, Vs, k0, p.Nk);
        mt = -INFINITY;
#pragma unroll
        for (int kk = 0; kk < DF32_KT; ++kk) {
            float a = 0.f;
#pragma unroll
            for (int d = 0; d < 32; ++d) a = fmaf(q2[d], K2s[kk][d], a);
            a *= p.scale;
            s[kk] = (k0 + kk < p.Nk) ? a : -INFINITY;
            mt = fmaxf(mt, s[kk]);
        }
        diff_f32_softmax_step(s, mt, m2, l2, a2, Vs, k0, p.Nk);
    }
    if (!active) return;
    const int64_t bh = (int64_t)b * p.H + h;
    if (p.lse1) {
        p.lse1[bh * p.Nq + q] = m1 + logf(l1);
        p.lse2[bh * p.Nq + q] = m2 + logf(l2);
    }
    const float inv1 = 1.0f / l1, inv2 = 1.0f / l2;
    float ss = 0.f;
#pragma unroll
    for (int d = 0; d < 64; ++d) {
        a1[d] *= inv1;
        a2[d] *= inv2;
        const float a = a1[d] - p.lambda * a2[d];   // channels >= DV are exactly zero
        ss = fmaf(a, a, ss);
    }
    const float rr = 1.0f / sqrtf(ss / (float)DV + p.eps);
    float* op = (float*)p.O + (int64_t)b * p.o_sb + (int64_t)q * p.o_sn + (int64_t)h * p.o_sh;
    const int64_t arow = (((int64_t)b * p.Nq + q) * p.H + h) * DV;
#pragma unroll
    for (int d = 0; d < 64; ++d)
        if (d < DV) {
            const float a = a1[d] - p.lambda * a2[d];
            op[d] = ((a * rr) * p.w[d]) * p.out_scale;
            if (p.A1) {
                ((float*)p.A1)[arow + d] = a1[d];
                ((float*)p.A2)[arow + d] = a2[d];
            }
        }
}

extern "C" int uc_diff_attention_fwd(const uc_diff_attention_desc* desc, uc_stream_t stream) {
    const char* fn = "uc_diff_attention_fwd";
    UC_REQUIRE(desc, "%s: null descriptor", fn);
    const uc_diff_attention_desc& d = *desc;
    UC_REQUIRE(d.dtype == UC_F32 || d.dtype == UC_BF16, "%s: unsupported dtype %d (UC_F32 or UC_BF16)", fn, d.dtype);
    UC_REQUIRE(d.Q && d.K && d.V && d.O && d.subln_w, "%s: null pointer", fn);
    UC_REQUIRE(d.B > 0 && d.H > 0 && d.Nq > 0 && d.Nk > 0 && d.Dqk > 0, "%s: bad shape", fn);
    UC_REQUIRE(d.H <= 65535 && d.B <= 65535, "%s: B and H must fit a grid dimension", fn);
    UC_REQUIRE(d.Dqk <= 32, "%s: Q/K head_dim %d with V head_dim %d is not supported: differential attention runs Q/K head_dim <= 32 "
               "(V head_dim <= 64); head_dim-128 attention does not exist in this library", fn, d.Dqk, 2 * d.Dqk);
    const int nsaves = (d.lse1 != nullptr) + (d.lse2 != nullptr) + (d.A1 != nullptr) + (d.A2 != nullptr);
    UC_REQUIRE(!d.training || nsaves == 4, "%s: training needs the four saves lse1, lse2, A1, A2 (got %d of them)", fn, nsaves);
    UC_REQUIRE(nsaves == 0 || nsaves == 4, "%s: the saves lse1, lse2, A1, A2 come together or not at all (got %d of them)", fn, nsaves);
    if (d.dtype == UC_BF16) {
        UC_REQUIRE(d.Dqk == 32, "%s(bf16): Q/K head_dim must be 32 (got %d)", fn, d.Dqk);
        UC_REQUIRE(d.v_layout == UC_V_PACKED_T, "%s(bf16): V must be in the packed VT layout (uc_vt_pack)", fn);
        UC_REQUIRE(d.q_sb % 8 == 0 && d.q_sn % 8 == 0 && d.q_sh % 8 == 0 && d.k_sb % 8 == 0 && d.k_sn % 8 == 0 && d.k_sh % 8 == 0,
                   "%s(bf16): Q/K strides must be multiples of 8 elements", fn);
        UC_REQUIRE(d.o_sb % 4 == 0 && d.o_sn % 4 == 0 && d.o_sh % 4 == 0, "%s(bf16): O strides must be multiples of 4", fn);
        UC_REQUIRE(((uintptr_t)d.Q % 16 == 0) && ((uintptr_t)d.K % 16 == 0) && ((uintptr_t)d.V % 16 == 0) && ((uintptr_t)d.O % 8 == 0) &&
                   ((uintptr_t)d.subln_w % 16 == 0) && ((uintptr_t)d.A1 % 8 == 0) && ((uintptr_t)d.A2 % 8 == 0), "%s(bf16): pointer alignment", fn);
    } else {
        UC_REQUIRE(d.Dqk % 4 == 0, "%s(f32): Q/K head_dim must be a multiple of 4 (got %d)", fn, d.Dqk);
        UC_REQUIRE(d.v_layout == UC_V_ROWMAJOR, "%s(f32): V must be row-major", fn);
    }
    DiffParams p;
    p.Q = d.Q; p.K = d.K; p.V = d.V; p.O = d.O; p.A1 = d.A1; p.A2 = d.A2; p.lse1 = d.lse1; p.lse2 = d.lse2; p.w = d.subln_w;
    p.B = d.B; p.H = d.H; p.Nq = d.Nq; p.Nk = d.Nk; p.Dqk = d.Dqk;
    p.q_sb = d.q_sb; p.q_sn = d.q_sn; p.q_sh = d.q_sh; p.k_sb = d.k_sb; p.k_sn = d.k_sn; p.k_sh = d.k_sh;
    p.v_sb = d.v_sb; p.v_sn = d.v_sn; p.v_sh = d.v_sh; p.o_sb = d.o_sb; p.o_sn = d.o_sn; p.o_sh = d.o_sh;
    p.npad = (d.Nk + 63) / 64 * 64;
    p.scale = d.scale; p.lambda = d.lambda_full; p.eps = d.rms_eps; p.out_scale = d.out_scale;
    const dim3 grid((unsigned)((d.Nq + 127) / 128), (unsigned)d.H, (unsigned)d.B);
    if (d.dtype == UC_BF16) hipLaunchKernelGGL(diff_attn_bf16_kernel, grid, dim3(256), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(diff_attn_f32_kernel, grid, dim3(128), 0, (hipStream_t)stream, p);
    UC_CHECK_LAUNCH(fn);
    return UC_OK;
}

// ---------------------------------------------------------------------------------------
// Backward of the combine step.  One wave per row (b, n, h), lane = channel; a workgroup's four waves walk a fixed set of rows in a
// fixed order, the four partial sums are added in wave order, and a second one-workgroup kernel adds the per-workgroup partials in
// index order: dw and dlambda have the same bits on every run (no float atomics).
// ---------------------------------------------------------------------------------------
#define DCB_SLOTS 65   // 64 channels of dw + dlambda

static inline int diff_combine_blocks(int64_t rows) {
    const int64_t n = (rows + 31) / 32;   // >= 8 rows per wave
    return (int)(n < 1 ? 1 : (n > 512 ? 512 : n));
}

template <typename Tag>
__global__ __launch_bounds__(256) void diff_combine_bwd_kernel(const typename Tag::storage* __restrict__ dY, const typename Tag::storage* __restrict__ A1,
                                                               const typename Tag::storage* __restrict__ A2, typename Tag::storage* __restrict__ dA1,
                                                               typename Tag::storage* __restrict__ dA2, const float* __restrict__ w,
                                                               float* __restrict__ partial, int64_t rows, int N, int H, int D, int64_t sb,
                                                               int64_t sn, int64_t sh, float lambda, float eps, float out_scale) {
    __shared__ float red[4][DCB_SLOTS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool on = lane < D;
    const float wl = on ? w[lane] : 0.f;
    const float invD = 1.0f / (float)D;
    float dw_acc = 0.f, dl_acc = 0.f;
    for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < rows; row += (int64_t)gridDim.x * 4) {
        const int hh = (int)(row % H);
        const int64_t bn = row / H;
        const int n = (int)(bn % N);
        const int64_t bb = bn / N;
        float a1 = 0.f, a2 = 0.f, dy = 0.f;
        if (on) {
            a1 = Tag::load(A1 + row * D + lane);
            a2 = Tag::load(A2 + row * D + lane);
            dy = Tag::load(dY + bb * sb + (int64_t)n * sn + (int64_t)hh * sh + lane);
        }
        const float a = a1 - lambda * a2;
        const float r = 1.0f / sqrtf(wave_sum(a * a) * invD + eps);
        const float g = dy * wl * out_scale;
        const float ga = wave_sum(g * a);
        const float da = r * g - (r * r * r) * a * (ga * invD);
        dw_acc += dy * (a * r) * out_scale;
        dl_acc -= da * a2;
        if (on) {
            Tag::store(dA1 + row * D + lane, da);
            Tag::store(dA2 + row * D + lane, -lambda * da);
        }
    }
    const float dl = wave_sum(dl_acc);
    red[wave][lane] = dw_acc;
    if (lane == 0) red[wave][64] = dl;
    __syncthreads();
    if (threadIdx.x < DCB_SLOTS) {
        const int t = threadIdx.x;
        partial[(int64_t)blockIdx.x * DCB_SLOTS + t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
    }
}

__global__ __launch_bounds__(128) void diff_combine_reduce_kernel(const float* __restrict__ partial, int nblk, int D, float* __restrict__ dw,
                                                                  float* __restrict__ dlambda) {
    const int t = threadIdx.x;
    if (t >= DCB_SLOTS) return;
    float s = 0.f;
    for (int i = 0; i < nblk; ++i) s += partial[(int64_t)i * DCB_SLOTS + t];
    if (t < D) dw[t] = s;
    else if (t == 64) dlambda[0] = s;
}

extern "C" int64_t uc_diff_attention_combine_ws_bytes(int64_t rows) {
    return (int64_t)diff_combine_blocks(rows) * DCB_SLOTS * (int64_t)sizeof(float);
}

extern "C" int uc_diff_attention_combine_bwd(const void* dY, const void* A1, const void* A2, void* dA1, void* dA2, const float* subln_w,
                                             float* dw, float* dlambda, float* ws, int dtype, int B, int N, int H, int D, int64_t dy_sb,
                                             int64_t dy_sn, int64_t dy_sh, float lambda_full, float rms_eps, float out_scale,
                                             uc_stream_t stream) {
    const char* fn = "uc_diff_attention_combine_bwd";
    UC_REQUIRE(dtype == UC_F32 || dtype == UC_BF16, "%s: unsupported dtype %d (UC_F32 or UC_BF16)", fn, dtype);
    UC_REQUIRE(dY && A1 && A2 && dA1 && dA2 && subln_w && dw && dlambda && ws, "%s: null pointer", fn);
    UC_REQUIRE(B > 0 && N > 0 && H > 0, "%s: bad shape", fn);
    UC_REQUIRE(D > 0 && D <= 64 && D % 4 == 0, "%s: D must be a multiple of 4, at most 64 (got %d)", fn, D);
    const int64_t rows = (int64_t)B * N * H;
    const int nblk = diff_combine_blocks(rows);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == UC_BF16)
        hipLaunchKernelGGL(diff_combine_bwd_kernel<BF16Tag>, dim3(nblk), dim3(256), 0, st, (const bf16_t*)dY, (const bf16_t*)A1, (const bf16_t*)A2,
                           (bf16_t*)dA1, (bf16_t*)dA2, subln_w, ws, rows, N, H, D, dy_sb, dy_sn, dy_sh, lambda_full, rms_eps, out_scale);
    else
        hipLaunchKernelGGL(diff_combine_bwd_kernel<F32Tag>, dim3(nblk), dim3(256), 0, st, (const float*)dY, (const float*)A1, (const float*)A2,
                           (float*)dA1, (float*)dA2, subln_w, ws, rows, N, H, D, dy_sb, dy_sn, dy_sh, lambda_full, rms_eps, out_scale);
    UC_CHECK_LAUNCH(fn);
    hipLaunchKernelGGL(diff_combine_reduce_kernel, dim3(1), dim3(128), 0, st, (const float*)ws, nblk, D, dw, dlambda);
    UC_CHECK_LAUNCH(fn);
    return UC_OK;
}
