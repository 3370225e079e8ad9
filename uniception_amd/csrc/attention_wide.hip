// Attention forward and backward for head_dim 80 and 96 on gfx950 (bf16, v_mfma_f32_32x32x16_bf16): the kernels and their two
// launchers.  uc_attention_fwd / uc_attention_bwd (attention.hip, attention_bwd.hip) validate, plan (attention_plan.h) and call a
// launcher where the plan names one of these kernels; nothing here validates or decides.
//
// The layout is that of attention_tile.h / attention_bwd.hip with D / 16 k-steps and three 32-channel output blocks:
//   forward   S^T = K . Q^T (KS = D / 16 k-steps), online softmax per lane pair, O^T += V^T . P^T into o[3];
//   dQ        S^T = K . Q^T, dP^T = V . dO^T, dQ^T += K^T . dS^T into dq[3];
//   dK / dV   S = Q . K^T, dP = dO . V^T, dV^T += dO^T . P, dK^T += Q^T . dS into dv[3], dk[3].
// Four waves, 128 rows per workgroup, tiles staged global -> VGPR -> LDS one tile ahead (two stages, one barrier per tile).
// LDS images:
//   row-major tiles (K in the forward; K, V, Q, dO in the backward): 64 rows of AW_RS = 208 bytes = 13 chunks of 16 B.  Chunks 0..11
//   hold channels 0..95 (head_dim 80: chunks 10 and 11 are written as zeros, so the third channel block's upper half multiplies
//   zeros), chunk 12 is padding that nothing reads.  An odd number of chunks per row makes the ds_read_b128 fragment loads (lane =
//   row, same chunk) conflict-free inside a 16-lane service group without a swizzle; the transposing reads (four consecutive rows x
//   32 B per 16-lane group) start 52 dwords apart: banks 0, 52, 40, 28 — conflict-free too.
//   VT tile (forward): 96 rows (channels; 80..95 zeros at head_dim 80) x 128 B of key positions, the tile_swz image of the 64-wide
//   kernels.
// Roundings: P (forward, dK / dV) and dS to bf16 before the second products, outputs to bf16; Q and K enter the score products as
// stored (scale * log2(e) is applied to the fp32 score, not folded into an operand).
#include "attention_tile.h"
#include "attention_wide.h"
#include <math.h>

constexpr int AW_RS = 208;                     // bytes per row of a row-major LDS tile
constexpr int AW_ROW_TILE = 64 * AW_RS;        // 13312
constexpr int AW_VT_TILE = 96 * 128;           // 12288
constexpr int AW_NB = 3;                       // 32-channel output blocks

struct AttnWideParams {
    const bf16_t *Q, *K, *VT;
    bf16_t* O;
    float* lse;
    int B, H, Nq, Nk, npad;
    int64_t q_sb, q_sn, q_sh, k_sb, k_sn, k_sh, o_sb, o_sn, o_sh;
    float scale;
};

struct AttnWideBwdParams {
    const bf16_t *Q, *K, *V, *O, *dO;
    const float* LSE;
    float* aux;                 // [B H][2][nq_pad]: -lse * log2(e) (absent queries: -1e30) | -delta (0), written by the dQ kernel
    int nq_pad;
    bf16_t *dQ, *dK, *dV;
    int B, H, Nq, Nk;
    int64_t q_sb, q_sn, q_sh, k_sb, k_sn, k_sh, v_sb, v_sn, v_sh, o_sb, o_sn, o_sh;
    int64_t dq_sb, dq_sn, dq_sh, dk_sb, dk_sn, dk_sh, dv_sb, dv_sn, dv_sh;
    float scale;
};

// One thread's share of a row-major [64 rows][D] tile: 3 of the 768 chunk slots (64 rows x 12 chunks).  Rows at or beyond n_rows
// re-read the last row (their scores are masked / their probabilities are 0); chunks at or beyond D / 8 are zeros.
template <int D>
struct AwRowStage {
    uint4 r[3];
    __device__ __forceinline__ void load(const bf16_t* base, const int64_t row_stride, const int row0, const int n_rows, const int tid) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int idx = tid + 256 * i, row = idx / 12, ch = idx - row * 12;
            int g = row0 + row;
            if (g >= n_rows) g = n_rows - 1;
            r[i] = make_uint4(0u, 0u, 0u, 0u);
            if (ch < D / 8) r[i] = *reinterpret_cast<const uint4*>(base + (int64_t)g * row_stride + ch * 8);
        }
    }
    __device__ __forceinline__ void store(char* tile, const int tid) const {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int idx = tid + 256 * i, row = idx / 12, ch = idx - row * 12;
            *reinterpret_cast<uint4*>(tile + row * AW_RS + ch * 16) = r[i];
        }
    }
};
// ... of the VT tile: 3 of the 768 slots (96 channel rows x 8 chunks of 8 key positions); rows at or beyond D are zeros
template <int D>
struct AwVtStage {
    uint4 r[3];
    __device__ __forceinline__ void load(const bf16_t* VTb, const int npad, const int k0, const int Nk, const int tid) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int idx = tid + 256 * i, row = idx >> 3, cc = idx & 7;
            r[i] = make_uint4(0u, 0u, 0u, 0u);
            if (row < D) r[i] = att_load_vt_chunk(VTb, row, npad, k0, cc, Nk);
        }
    }
    __device__ __forceinline__ void store(char* tile, const int tid) const {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int idx = tid + 256 * i, row = idx >> 3, cc = idx & 7;
            *reinterpret_cast<uint4*>(tile + tile_swz(row, cc)) = r[i];
        }
    }
};

// att_softmax_step (attention_tile.h) with three output blocks to rescale
template <class Probs>
__device__ __forceinline__ void aw_softmax_step(const float16_t (&s)[2], float& m_run, float& l_run, float16_t (&o)[AW_NB], const float c, Probs& pr) {
    float mt = s[0][0];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) mt = fmaxf(mt, s[kb][r]);
    mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
    const bool grow = (mt - m_run) * c > Probs::RESCALE_LOG2;
    if (__any(grow)) {
        const float m_new = fmaxf(m_run, mt);
        const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * c);
        m_run = m_new;
        l_run *= alpha;
#pragma unroll
        for (int db = 0; db < AW_NB; ++db)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[db][r] *= alpha;
    }
    const float mc = m_run * c;
    float psum = 0.f;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int g = 0; g < 16 / Probs::GROUP; ++g) {
            float e[Probs::GROUP];
#pragma unroll
            for (int j = 0; j < Probs::GROUP; ++j) {
                e[j] = __builtin_amdgcn_exp2f(fmaf(s[kb][g * Probs::GROUP + j], c, -mc));
                psum += e[j];
            }
            pr.put(kb, g, e);
        }
    l_run += psum;
}

// tr_operand (attention_bwd.hip) on an unswizzled AW_RS-byte-row tile: for the 32-channel block cb the lane (channel = 32 cb +
// (lane & 31), k half = lane >> 5) receives rows  slab16 * 16 + 4 * (lane >> 5) + {0,1,2,3, 8,9,10,11}.
__device__ __forceinline__ bf16x8_t aw_tr_operand(const char* tile, const int slab16, const int cb, const int lane) {
    const int jj = lane & 15;
    const int d0 = cb * 32 + (((lane >> 4) & 1) << 4);
    const int piece = jj & 3;
    const int row0 = slab16 * 16 + 4 * (lane >> 5) + (jj >> 2);
    const char* a0 = tile + row0 * AW_RS + d0 * 2 + piece * 8;
    const bf16x4_t lo = lds_read_tr16(a0), hi = lds_read_tr16(a0 + 8 * AW_RS);
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// store the lane's channels of a [3][16] accumulator (times f) to the bf16 row op: 4 consecutive channels per (db, g4), d < D only
template <int D>
__device__ __forceinline__ void aw_store_row(const float16_t (&a)[AW_NB], const float f, bf16_t* op, const int hi) {
#pragma unroll
    for (int db = 0; db < AW_NB; ++db)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            if (32 * db + 8 * g4 + 8 > D) continue;   // (compile time: head_dim 80 has no channels 80..95)
            const int d = att_frag_row(db, g4 * 4, hi);
            uint2 pk;
            pk.x = pack_bf16x2(a[db][g4 * 4 + 0] * f, a[db][g4 * 4 + 1] * f);
            pk.y = pack_bf16x2(a[db][g4 * 4 + 2] * f, a[db][g4 * 4 + 3] * f);
            *reinterpret_cast<uint2*>(op + d) = pk;
        }
}

// =================================================================================================================
// forward
// =================================================================================================================
template <int D>
__global__ __launch_bounds__(256) void attnw_fwd_kernel(AttnWideParams p) {
    constexpr int KS = D / 16, STAGE = AW_ROW_TILE + AW_VT_TILE;
    __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];   // 2 stages x (K rows | VT)
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int hi = lane >> 5, l31 = lane & 31;
    const int b = blockIdx.z, h = blockIdx.y;
    const int q0 = blockIdx.x * 128 + wave * 32;

    const bf16_t* Kb = p.K + (int64_t)b * p.k_sb + (int64_t)h * p.k_sh;
    const bf16_t* VTb = p.VT + ((int64_t)b * p.H + h) * D * (int64_t)p.npad;

    bf16x8_t qf[KS];   // Q^T fragments (B operand): lane (q = l31, hi) holds Q[q][16 s + 8 hi .. +7]
    {
        int q = q0 + l31;
        if (q >= p.Nq) q = p.Nq - 1;   // clamp; rows beyond Nq are never stored
        const bf16_t* qp = p.Q + (int64_t)b * p.q_sb + (int64_t)q * p.q_sn + (int64_t)h * p.q_sh + hi * 8;
#pragma unroll
        for (int s = 0; s < KS; ++s) qf[s] = *reinterpret_cast<const bf16x8_t*>(qp + 16 * s);
    }
    int r_off[4];   // VT fragment offsets
    att_frag_offsets(r_off, l31, hi);
    const int k_off = l31 * AW_RS + hi * 16;

    float16_t o[AW_NB];
#pragma unroll
    for (int db = 0; db < AW_NB; ++db) o[db] = (float16_t)(0.f);
    float m_run = ATT_MASKED, l_run = 0.f;
    const float c = p.scale * ATT_LOG2E;

    AwRowStage<D> stk;
    AwVtStage<D> stv;
    const int nt = (p.Nk + ATT_KV_TILE - 1) / ATT_KV_TILE;
    stk.load(Kb, p.k_sn, 0, p.Nk, tid);
    stv.load(VTb, p.npad, 0, p.Nk, tid);
    stk.store(smem, tid);
    stv.store(smem + AW_ROW_TILE, tid);
    __syncthreads();

    for (int t = 0; t < nt; ++t) {
        const int k0 = t * ATT_KV_TILE;
        if (t + 1 < nt) {
            stk.load(Kb, p.k_sn, k0 + ATT_KV_TILE, p.Nk, tid);
            stv.load(VTb, p.npad, k0 + ATT_KV_TILE, p.Nk, tid);
        }
        const char* sk = smem + (t & 1) * STAGE;
        const char* sv = sk + AW_ROW_TILE;

        float16_t s[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            s[kb] = (float16_t)(0.f);
#pragma unroll
            for (int st = 0; st < KS; ++st) {
                const bf16x8_t kf = *reinterpret_cast<const bf16x8_t*>(sk + k_off + kb * (32 * AW_RS) + st * 32);
                s[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[st], s[kb], 0, 0, 0);
            }
        }
        if (k0 + ATT_KV_TILE > p.Nk) att_mask_tail(s, k0, p.Nk, hi);
        AttProbsBf16 pr;
        aw_softmax_step(s, m_run, l_run, o, c, pr);
#pragma unroll
        for (int db = 0; db < AW_NB; ++db)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const bf16x8_t vf = *reinterpret_cast<const bf16x8_t*>(sv + r_off[g] + db * (32 * 128));
                o[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pr.pf[g], o[db], 0, 0, 0);
            }

        if (t + 1 < nt) {
            char* nx = smem + ((t + 1) & 1) * STAGE;
            stk.store(nx, tid);
            stv.store(nx + AW_ROW_TILE, tid);
        }
        __syncthreads();
    }

    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    const int q = q0 + l31;
    att_store_lse(p.lse, (int64_t)b * p.H + h, p.Nq, q, hi, m_run, p.scale, l_tot);
    if (q < p.Nq) aw_store_row<D>(o, 1.0f / l_tot, p.O + (int64_t)b * p.o_sb + (int64_t)q * p.o_sn + (int64_t)h * p.o_sh, hi);
}

// =================================================================================================================
// dQ: a workgroup owns 128 queries and streams 64-key K / V tiles.  Also leaves the per-query scalars of the dK / dV kernel in aux.
// =================================================================================================================
template <int D>
__global__ __launch_bounds__(256) void attnw_bwd_dq_kernel(AttnWideBwdParams p) {
    constexpr int KS = D / 16;
    __shared__ __attribute__((aligned(16))) char smem[4 * AW_ROW_TILE];   // 2 stages x (K rows | V rows)
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int hi = lane >> 5, l31 = lane & 31;
    const int nqt = (p.Nq + 127) / 128;
    const int bh = (int)blockIdx.x / nqt, tile = (int)blockIdx.x - bh * nqt;
    const int b = bh / p.H, h = bh - b * p.H;
    const int q0 = tile * 128 + wave * 32;
    int q = q0 + l31;
    const bool q_ok = q < p.Nq;
    if (!q_ok) q = p.Nq - 1;

    const bf16_t* Kb = p.K + (int64_t)b * p.k_sb + (int64_t)h * p.k_sh;
    const bf16_t* Vb = p.V + (int64_t)b * p.v_sb + (int64_t)h * p.v_sh;

    bf16x8_t qf[KS], dof[KS];
    float dlt = 0.f;   // delta[q] = sum_d dO[q, d] * O[q, d]
    {
        const bf16_t* qp = p.Q + (int64_t)b * p.q_sb + (int64_t)q * p.q_sn + (int64_t)h * p.q_sh + hi * 8;
        const bf16_t* dp = p.dO + (int64_t)b * p.o_sb + (int64_t)q * p.o_sn + (int64_t)h * p.o_sh + hi * 8;
        const bf16_t* op = p.O + (int64_t)b * p.o_sb + (int64_t)q * p.o_sn + (int64_t)h * p.o_sh + hi * 8;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            qf[s] = *reinterpret_cast<const bf16x8_t*>(qp + 16 * s);
            dof[s] = *reinterpret_cast<const bf16x8_t*>(dp + 16 * s);
            const bf16x8_t of = *reinterpret_cast<const bf16x8_t*>(op + 16 * s);
#pragma unroll
            for (int j = 0; j < 8; ++j) dlt = fmaf((float)of[j], (float)dof[s][j], dlt);
        }
        dlt += __shfl_xor(dlt, 32, 64);
    }
    const float c = p.scale * ATT_LOG2E;
    const float lse2 = p.LSE[((int64_t)b * p.H + h) * p.Nq + q] * ATT_LOG2E;
    if (hi == 0) {   // every query slot up to nq_pad gets its pair
        float* ax = p.aux + ((int64_t)b * p.H + h) * 2 * p.nq_pad + (q0 + l31);
        ax[0] = q_ok ? -lse2 : -1e30f;
        ax[p.nq_pad] = q_ok ? -dlt : 0.f;
    }

    float16_t dq[AW_NB];
#pragma unroll
    for (int db = 0; db < AW_NB; ++db) dq[db] = (float16_t)(0.f);
    const int k_off = l31 * AW_RS + hi * 16;

    AwRowStage<D> stk, stv;
    const int nt = (p.Nk + 63) / 64;
    stk.load(Kb, p.k_sn, 0, p.Nk, tid);
    stv.load(Vb, p.v_sn, 0, p.Nk, tid);
    stk.store(smem, tid);
    stv.store(smem + AW_ROW_TILE, tid);
    __syncthreads();

    for (int t = 0; t < nt; ++t) {
        const int k0 = t * 64;
        if (t + 1 < nt) {
            stk.load(Kb, p.k_sn, k0 + 64, p.Nk, tid);
            stv.load(Vb, p.v_sn, k0 + 64, p.Nk, tid);
        }
        const char* sk = smem + (t & 1) * 2 * AW_ROW_TILE;
        const char* sv = sk + AW_ROW_TILE;
        const bool tail = k0 + 64 > p.Nk;

        bf16x8_t dsf[4];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            float16_t s = (float16_t)(0.f), dp = (float16_t)(0.f);
#pragma unroll
            for (int st = 0; st < KS; ++st) {
                const bf16x8_t kf = *reinterpret_cast<const bf16x8_t*>(sk + k_off + kb * (32 * AW_RS) + st * 32);
                const bf16x8_t vf = *reinterpret_cast<const bf16x8_t*>(sv + k_off + kb * (32 * AW_RS) + st * 32);
                s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[st], s, 0, 0, 0);        // Q K^T
                dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, dof[st], dp, 0, 0, 0);     // dO V^T
            }
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                float e[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int r = hf * 8 + j;
                    float pv = __builtin_amdgcn_exp2f(fmaf(s[r], c, -lse2));
                    if (tail && k0 + att_frag_row(kb, r, hi) >= p.Nk) pv = 0.f;
                    e[j] = pv * (dp[r] - dlt);
                }
                dsf[kb * 2 + hf] = att_pack_bf16x8(e);
            }
        }
#pragma unroll
        for (int db = 0; db < AW_NB; ++db)
#pragma unroll
            for (int g = 0; g < 4; ++g)   // K^T[d block db, 16-key slab g]: clamped duplicate rows of a tail tile meet dS = 0
                dq[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(aw_tr_operand(sk, g, db, lane), dsf[g], dq[db], 0, 0, 0);

        if (t + 1 < nt) {
            char* nx = smem + ((t + 1) & 1) * 2 * AW_ROW_TILE;
            stk.store(nx, tid);
            stv.store(nx + AW_ROW_TILE, tid);
        }
        __syncthreads();
    }
    if (q_ok) aw_store_row<D>(dq, p.scale, p.dQ + (int64_t)b * p.dq_sb + (int64_t)q * p.dq_sn + (int64_t)h * p.dq_sh, hi);
}

// =================================================================================================================
// dK, dV: a workgroup owns 128 keys and streams 64-query Q / dO tiles
// =================================================================================================================
template <int D>
__global__ __launch_bounds__(256) void attnw_bwd_dkv_kernel(AttnWideBwdParams p) {
    constexpr int KS = D / 16;
    __shared__ __attribute__((aligned(16))) char smem[4 * AW_ROW_TILE + 1024];   // 2 stages x (Q rows | dO rows) + 2 x (-lse2[64] | -delta[64])
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int hi = lane >> 5, l31 = lane & 31;
    const int nkt = (p.Nk + 127) / 128;
    const int bh = (int)blockIdx.x / nkt, tile = (int)blockIdx.x - bh * nkt;
    const int b = bh / p.H, h = bh - b * p.H;
    const int key0 = tile * 128 + wave * 32;
    int key = key0 + l31;
    const bool key_ok = key < p.Nk;
    if (!key_ok) key = p.Nk - 1;

    const bf16_t* Qb = p.Q + (int64_t)b * p.q_sb + (int64_t)h * p.q_sh;
    const bf16_t* dOb = p.dO + (int64_t)b * p.o_sb + (int64_t)h * p.o_sh;
    const float* ax_b = p.aux + ((int64_t)b * p.H + h) * 2 * p.nq_pad;
    float* s_aux = reinterpret_cast<float*>(smem + 4 * AW_ROW_TILE);   // [stage][-lse2 64 | -delta 64]

    bf16x8_t kf[KS], vf[KS];   // B operands: lane key = l31, channels 16 s + 8 hi .. +7
    {
        const bf16_t* kp = p.K + (int64_t)b * p.k_sb + (int64_t)key * p.k_sn + (int64_t)h * p.k_sh + hi * 8;
        const bf16_t* vp = p.V + (int64_t)b * p.v_sb + (int64_t)key * p.v_sn + (int64_t)h * p.v_sh + hi * 8;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            kf[s] = *reinterpret_cast<const bf16x8_t*>(kp + 16 * s);
            vf[s] = *reinterpret_cast<const bf16x8_t*>(vp + 16 * s);
        }
    }
    const float c = p.scale * ATT_LOG2E;
    float16_t dk[AW_NB], dv[AW_NB];
#pragma unroll
    for (int db = 0; db < AW_NB; ++db) { dk[db] = (float16_t)(0.f); dv[db] = (float16_t)(0.f); }
    const int q_off = l31 * AW_RS + hi * 16;

    AwRowStage<D> stq, std_;
    float ax0 = 0.f, ax1 = 0.f;   // threads 0..63: the staged per-query scalars
    auto load_aux = [&](int q0) {
        if (tid < 64) {
            const int qq = q0 + tid;
            ax0 = qq < p.Nq ? ax_b[qq] : -1e30f;   // absent query: P = exp2(-1e30) = 0
            ax1 = qq < p.Nq ? ax_b[p.nq_pad + qq] : 0.f;
        }
    };
    auto store_aux = [&](int stage) {
        if (tid < 64) { s_aux[stage * 128 + tid] = ax0; s_aux[stage * 128 + 64 + tid] = ax1; }
    };
    const int nt = (p.Nq + 63) / 64;
    stq.load(Qb, p.q_sn, 0, p.Nq, tid);
    std_.load(dOb, p.o_sn, 0, p.Nq, tid);
    load_aux(0);
    stq.store(smem, tid);
    std_.store(smem + AW_ROW_TILE, tid);
    store_aux(0);
    __syncthreads();

    for (int t = 0; t < nt; ++t) {
        const int q0 = t * 64;
        if (t + 1 < nt) {
            stq.load(Qb, p.q_sn, q0 + 64, p.Nq, tid);
            std_.load(dOb, p.o_sn, q0 + 64, p.Nq, tid);
            load_aux(q0 + 64);
        }
        const char* sq = smem + (t & 1) * 2 * AW_ROW_TILE;
        const char* sd = sq + AW_ROW_TILE;
        const float* s_nl = s_aux + (t & 1) * 128;
        const float* s_nd = s_nl + 64;

#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
            float16_t s = (float16_t)(0.f), dp = (float16_t)(0.f);
#pragma unroll
            for (int st = 0; st < KS; ++st) {
                const bf16x8_t qa = *reinterpret_cast<const bf16x8_t*>(sq + q_off + qb * (32 * AW_RS) + st * 32);
                const bf16x8_t da = *reinterpret_cast<const bf16x8_t*>(sd + q_off + qb * (32 * AW_RS) + st * 32);
                s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qa, kf[st], s, 0, 0, 0);      // S[q rows, key cols]
                dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(da, vf[st], dp, 0, 0, 0);    // dP[q rows, key cols]
            }
            bf16x8_t pfr[2], dsfr[2];
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                float pe[8], de[8];
#pragma unroll
                for (int k4 = 0; k4 < 2; ++k4) {
                    // accumulator registers 4k .. 4k+3 = queries qb*32 + 8k + 4hi .. +3: one 16-byte LDS read each
                    const float4_t nl = *reinterpret_cast<const float4_t*>(s_nl + qb * 32 + 8 * (2 * hf + k4) + 4 * hi);
                    const float4_t nd = *reinterpret_cast<const float4_t*>(s_nd + qb * 32 + 8 * (2 * hf + k4) + 4 * hi);
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) {
                        const int r = hf * 8 + k4 * 4 + jj;
                        const float pv = __builtin_amdgcn_exp2f(fmaf(s[r], c, nl[jj]));
                        pe[k4 * 4 + jj] = pv;
                        de[k4 * 4 + jj] = pv * (dp[r] + nd[jj]);
                    }
                }
                pfr[hf] = att_pack_bf16x8(pe);
                dsfr[hf] = att_pack_bf16x8(de);
            }
#pragma unroll
            for (int db = 0; db < AW_NB; ++db)
#pragma unroll
                for (int hf = 0; hf < 2; ++hf) {
                    const int g = qb * 2 + hf;   // queries beyond Nq are clamped duplicates in the tiles; their P / dS columns are exactly 0
                    dv[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(aw_tr_operand(sd, g, db, lane), pfr[hf], dv[db], 0, 0, 0);    // dV^T[d, key]
                    dk[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(aw_tr_operand(sq, g, db, lane), dsfr[hf], dk[db], 0, 0, 0);   // dK^T[d, key]
                }
        }

        if (t + 1 < nt) {
            char* nx = smem + ((t + 1) & 1) * 2 * AW_ROW_TILE;
            stq.store(nx, tid);
            std_.store(nx + AW_ROW_TILE, tid);
            store_aux((t + 1) & 1);
        }
        __syncthreads();
    }
    if (key_ok) {
        aw_store_row<D>(dk, p.scale, p.dK + (int64_t)b * p.dk_sb + (int64_t)key * p.dk_sn + (int64_t)h * p.dk_sh, hi);
        aw_store_row<D>(dv, 1.0f, p.dV + (int64_t)b * p.dv_sb + (int64_t)key * p.dv_sn + (int64_t)h * p.dv_sh, hi);
    }
}

// =================================================================================================================
// launchers: uc_attention_fwd / uc_attention_bwd have validated the descriptor and planned the launch (attention_plan.h)
// =================================================================================================================
int uc_attention_wide_fwd_launch(const uc_attention_desc& d, const AttnFwdPlan& plan, uc_stream_t stream) {
    AttnWideParams p;
    p.Q = (const bf16_t*)d.Q; p.K = (const bf16_t*)d.K; p.VT = (const bf16_t*)d.V; p.O = (bf16_t*)d.O; p.lse = d.lse;
    p.B = d.B; p.H = d.H; p.Nq = d.Nq; p.Nk = d.Nk; p.npad = (d.Nk + 63) / 64 * 64;
    p.q_sb = d.q_sb; p.q_sn = d.q_sn; p.q_sh = d.q_sh; p.k_sb = d.k_sb; p.k_sn = d.k_sn; p.k_sh = d.k_sh;
    p.o_sb = d.o_sb; p.o_sn = d.o_sn; p.o_sh = d.o_sh; p.scale = d.scale;
    const dim3 grid(plan.grid[0], plan.grid[1], plan.grid[2]), block(plan.block);
    hipStream_t st = (hipStream_t)stream;
    if (plan.kernel == UC_AF_BF16_80) hipLaunchKernelGGL(attnw_fwd_kernel<80>, grid, block, 0, st, p);
    else hipLaunchKernelGGL(attnw_fwd_kernel<96>, grid, block, 0, st, p);
    UC_CHECK_LAUNCH("uc_attention_fwd");
    return UC_OK;
}

int uc_attention_wide_bwd_launch(const uc_attention_bwd_desc& d, const AttnBwdPlan& plan, uc_stream_t stream) {
    AttnWideBwdParams p;
    p.Q = (const bf16_t*)d.Q; p.K = (const bf16_t*)d.K; p.V = (const bf16_t*)d.V; p.O = (const bf16_t*)d.O; p.dO = (const bf16_t*)d.dO;
    p.LSE = d.LSE; p.aux = d.delta; p.nq_pad = (d.Nq + 127) / 128 * 128;
    p.dQ = (bf16_t*)d.dQ; p.dK = (bf16_t*)d.dK; p.dV = (bf16_t*)d.dV;
    p.B = d.B; p.H = d.H; p.Nq = d.Nq; p.Nk = d.Nk;
    p.q_sb = d.q_sb; p.q_sn = d.q_sn; p.q_sh = d.q_sh; p.k_sb = d.k_sb; p.k_sn = d.k_sn; p.k_sh = d.k_sh; p.v_sb = d.v_sb; p.v_sn = d.v_sn;
    p.v_sh = d.v_sh; p.o_sb = d.o_sb; p.o_sn = d.o_sn; p.o_sh = d.o_sh; p.dq_sb = d.dq_sb; p.dq_sn = d.dq_sn; p.dq_sh = d.dq_sh;
    p.dk_sb = d.dk_sb; p.dk_sn = d.dk_sn; p.dk_sh = d.dk_sh; p.dv_sb = d.dv_sb; p.dv_sn = d.dv_sn; p.dv_sh = d.dv_sh; p.scale = d.scale;
    hipStream_t st = (hipStream_t)stream;
    const dim3 gq(plan.dq_grid[0]), gkv(plan.dkv_grid[0]), block(plan.block);
    if (plan.dq == UC_AB_DQ80) hipLaunchKernelGGL(attnw_bwd_dq_kernel<80>, gq, block, 0, st, p);
    else hipLaunchKernelGGL(attnw_bwd_dq_kernel<96>, gq, block, 0, st, p);
    if (plan.dkv == UC_AB_DKV80) hipLaunchKernelGGL(attnw_bwd_dkv_kernel<80>, gkv, block, 0, st, p);
    else hipLaunchKernelGGL(attnw_bwd_dkv_kernel<96>, gkv, block, 0, st, p);
    UC_CHECK_LAUNCH("uc_attention_bwd");
    return UC_OK;
}
