// Fused scaled-dot-product attention for gfx950.
//
// attn_bf16_kernel — flash-style, head_dim 64, v_mfma_f32_32x32x16_bf16.
//   Workgroup = 4 wavefronts = 128 query rows of one (batch, head); each wave owns 32 queries.  The per-key-tile step and its operand
//   layout are those of attention_tile.h; here K and VT tiles are staged global -> VGPR -> LDS one tile ahead (double-buffered,
//   XOR-swizzled 128-byte rows, one barrier per tile).
//
// attn_f32_kernel — verification mode: one thread per query row, fp32 FMA chains, expf.
#include "attention_tile.h"
#include "knobs.h"
#include "attention_p64.h"
#include "attention_plan.h"
#include "attention_wide.h"
#include <stdlib.h>

struct AttnParams {
    const void* Q;
    const void* K;
    const void* V;
    void* O;
    int B, H, Nq, Nk, D;
    int64_t q_sb, q_sn, q_sh, k_sb, k_sn, k_sh, v_sb, v_sn, v_sh, o_sb, o_sn, o_sh;
    int npad;     // VT row length
    float scale;
    float* lse;   // optional [B,H,Nq]: log-sum-exp of the scaled scores (saved for the backward)
    uc_fastdiv dGroup, dNq, dH;   // exact fast division by 8*nq, nq, H (workgroup -> (query tile, batch, head) in the DMA kernel)
    int prio_young;               // eight-wave workgroups: s_setprio 1 for waves 4-7 (the younger half loses every VALU arbitration to the older one)
    UcDropout drop;               // attention dropout (uc_attention_fwd with drop_p > 0; thr 0 elsewhere)
};

// the body of attn_bf16_kernel for the 128 queries from q0w of (batch b, head h): also what attn_bf16_fixup_kernel recomputes a
// flagged block of the persistent kernel with (attention_p64.h)
// DROP: attention dropout (training with attn_drop > 0): the row sum — the softmax's normalisation — takes every probability, the
// P^T operand of O^T += V^T P^T only the kept ones, scaled by 1 / (1 - p): O = (P o mask / (1 - p)) V, the reference's
// attn_drop(softmax(...)) @ v.  The LSE is that of the undropped scores.
template <bool DROP = false>
__device__ __forceinline__ void attn_bf16_body(const AttnParams& p, const int b, const int h, const int q0w, char* smem) {
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int hi = lane >> 5;
    const int l31 = lane & 31;
    const int q0 = q0w + wave * 32;

    const bf16_t* Qb = (const bf16_t*)p.Q + (int64_t)b * p.q_sb + (int64_t)h * p.q_sh;
    const bf16_t* Kb = (const bf16_t*)p.K + (int64_t)b * p.k_sb + (int64_t)h * p.k_sh;
    const bf16_t* VTb = (const bf16_t*)p.V + ((int64_t)b * p.H + h) * 64 * (int64_t)p.npad;

    // ---- Q^T fragments (B operand): lane (q = l31, hi) holds Q[q][16s + 8hi .. +7], s = 0..3 ----
    bf16x8_t qf[4];
    {
        int q = q0 + l31;
        if (q >= p.Nq) q = p.Nq - 1;  // clamp; rows beyond Nq are never stored
        const bf16_t* qp = Qb + (int64_t)q * p.q_sn + hi * 8;
#pragma unroll
        for (int s = 0; s < 4; ++s) qf[s] = *reinterpret_cast<const bf16x8_t*>(qp + 16 * s);
    }

    // ---- staging assignment: 512 16-byte chunks per tile, 2 per thread ----
    const int cc = tid & 7;     // chunk column
    const int sr = tid >> 3;    // row 0..31 (+32)
    uint4 rk0, rk1, rv0, rv1;   // named (not arrays) so they stay in VGPRs
    auto load_k = [&](int k0, int row) -> uint4 {
        int key = k0 + row;
        if (key >= p.Nk) key = p.Nk - 1;  // clamped keys are masked in the softmax
        return *reinterpret_cast<const uint4*>(Kb + (int64_t)key * p.k_sn + cc * 8);
    };
    auto load_v = [&](int k0, int row) -> uint4 { return att_load_vt_chunk(VTb, row, p.npad, k0, cc, p.Nk); };
#define ATT_STAGE_LOAD(k0_)                 \
    do {                                    \
        rk0 = load_k((k0_), sr);            \
        rk1 = load_k((k0_), sr + 32);       \
        rv0 = load_v((k0_), sr);            \
        rv1 = load_v((k0_), sr + 32);       \
    } while (0)
    // loop-invariant LDS byte offsets: rows r and r+32 share the swizzle key, so one offset + an immediate serves both
    const int w_off = tile_swz(sr, cc);
#define ATT_STAGE_WRITE(buf_)                                                          \
    do {                                                                               \
        char* sk_ = smem + (buf_) * 2 * ATT_TILE_BYTES + w_off;                        \
        *reinterpret_cast<uint4*>(sk_) = rk0;                                          \
        *reinterpret_cast<uint4*>(sk_ + 32 * 128) = rk1;                               \
        *reinterpret_cast<uint4*>(sk_ + ATT_TILE_BYTES) = rv0;                         \
        *reinterpret_cast<uint4*>(sk_ + ATT_TILE_BYTES + 32 * 128) = rv1;              \
    } while (0)
    int r_off[4];   // fragment read offsets (K and VT tiles alike)
    att_frag_offsets(r_off, l31, hi);

    float16_t o[2];   // O^T accumulators: d-block x (16 regs): d = att_frag_row(db, r, hi), q = l31
    o[0] = (float16_t)(0.f);
    o[1] = (float16_t)(0.f);
    float m_run = ATT_MASKED;   // running max of raw scores (shared by the lane pair)
    float l_run = 0.f;      // lane-partial running sum
    const float c = p.scale * ATT_LOG2E;  // scale * log2(e)
    unsigned dk1 = 0, dk2 = 0;
    if constexpr (DROP) uc_drop_keys(p.drop, (unsigned)(b * p.H + h), dk1, dk2);

    const int nt = (p.Nk + ATT_KV_TILE - 1) / ATT_KV_TILE;
    ATT_STAGE_LOAD(0);
    ATT_STAGE_WRITE(0);
    __syncthreads();

    for (int t = 0; t < nt; ++t) {
        const int buf = t & 1;
        const int k0 = t * ATT_KV_TILE;
        if (t + 1 < nt) ATT_STAGE_LOAD(k0 + ATT_KV_TILE);
        const char* sk = smem + buf * 2 * ATT_TILE_BYTES;
        const char* sv = sk + ATT_TILE_BYTES;

        float16_t s[2];
        att_scores_bf16(s, sk, r_off, qf);
        if (k0 + ATT_KV_TILE > p.Nk) att_mask_tail(s, k0, p.Nk, hi);
        // ---- online softmax (per query = per lane pair) ----
        std::conditional_t<DROP, AttProbsBf16Drop, AttProbsBf16> pr;
        if constexpr (DROP) { pr.k1 = dk1; pr.k2 = dk2; pr.q = (unsigned)(q0 + l31); pr.k0 = k0; pr.hi = hi; pr.drop = p.drop; }
        att_softmax_step(s, m_run, l_run, o, c, pr);
        att_pv_bf16(o, sv, r_off, pr.pf);

        if (t + 1 < nt) ATT_STAGE_WRITE(buf ^ 1);
        __syncthreads();
    }

    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    const int q = q0 + l31;
    att_store_lse(p.lse, (int64_t)b * p.H + h, p.Nq, q, hi, m_run, p.scale, l_tot);
    if (q < p.Nq) att_store_rows_direct(o, 1.0f / l_tot, (bf16_t*)p.O + (int64_t)b * p.o_sb + (int64_t)q * p.o_sn + (int64_t)h * p.o_sh, hi);
}

__global__ __launch_bounds__(256) void attn_bf16_kernel(AttnParams p) {
    __shared__ __attribute__((aligned(16))) char smem[4 * ATT_TILE_BYTES];  // 2 stages x (K tile + VT tile)
    attn_bf16_body(p, (int)blockIdx.z, (int)blockIdx.y, (int)blockIdx.x * 128, smem);
}
__global__ __launch_bounds__(256) void attn_bf16_drop_kernel(AttnParams p) {
    __shared__ __attribute__((aligned(16))) char smem[4 * ATT_TILE_BYTES];
    attn_bf16_body<true>(p, (int)blockIdx.z, (int)blockIdx.y, (int)blockIdx.x * 128, smem);
}

// ---------------------------------------------------------------------------------------
// attn_bf16_fixup_kernel — launched behind attn_bf16_p64_kernel: that kernel takes every exponential against the row maximum of an
// item's FIRST 32 keys and flags a 64-query block whose row sums left [2^-100, 2^100] (a score ~69 nats above / below that
// maximum: P or O may have over- / underflowed) with a sentinel in the block's first output word.  One thread per block reads
// that word; a flagged block is recomputed by the whole workgroup with the exact online softmax above (the 128 queries from the
// block's first one: the second half re-does an unflagged neighbour, or finds it flagged and is simply ahead of its own scan).
// Flags are rare by construction; the scan is one 4-byte load per 64 x 64 outputs.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void attn_bf16_fixup_kernel(AttnParams p) {
    __shared__ __attribute__((aligned(16))) char smem[4 * ATT_TILE_BYTES];
    __shared__ int s_list[256];
    __shared__ int s_cnt;
    const int nblk = (p.Nq + 63) >> 6;
    const long long total = (long long)p.B * p.H * nblk;
    for (long long c0 = (long long)blockIdx.x * 256; c0 < total; c0 += (long long)gridDim.x * 256) {
        if (threadIdx.x == 0) s_cnt = 0;
        __syncthreads();
        const long long id = c0 + threadIdx.x;
        if (id < total) {
            const int blk = (int)(id % nblk), bh = (int)(id / nblk), b = bh / p.H, h = bh - b * p.H;
            const unsigned* w = reinterpret_cast<const unsigned*>((const bf16_t*)p.O + (int64_t)b * p.o_sb + (int64_t)(blk * 64) * p.o_sn + (int64_t)h * p.o_sh);
            if (__builtin_nontemporal_load(w) == P64_SENTINEL) s_list[atomicAdd(&s_cnt, 1)] = (int)threadIdx.x;
        }
        __syncthreads();
        const int n = s_cnt;
        for (int i = 0; i < n; ++i) {
            const long long fid = c0 + s_list[i];
            const int blk = (int)(fid % nblk), bh = (int)(fid / nblk), b = bh / p.H, h = bh - b * p.H;
            __syncthreads();                              // (the body's LDS ring and s_list: the previous body is done)
            attn_bf16_body(p, b, h, blk * 64, smem);
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------
// attn_bf16_dma_kernel — the same algorithm (the VT pad positions of a ragged last tile must hold zeros: uc_vt_pack and
// ops.vt_buffer guarantee it) with the K and
// VT tiles staged by buffer-addressed LDS-DMA instead of global -> VGPR -> LDS.  The register-staged kernel needs 184
// registers (152 VGPR + the score accumulators pushed into 32 AGPRs: 2 waves per SIMD, 64 v_accvgpr moves per key tile);
// without the 16 staging registers, the per-chunk tail masks of V and the per-tile address math this one fits the 128-register budget
// of 4 waves per SIMD.  Descriptors: K rows / VT rows of this (batch, head); the per-lane byte offsets are loop
// invariant, the tile advance is a wave-uniform soffset.
// ---------------------------------------------------------------------------------------
// What bounds it (round 2, tools/scratch/probe_attn_anatomy.py and its SQ counters, B = 64, H = 16, N = 1024): the costs of the exp2
// work and of the PV products are ADDITIVE (-18 % without the exps, -20 % without the PV MFMAs, -2 % without the per-tile
// barrier; static priorities or a start stagger per workgroup slot: nothing).  SQ_ACTIVE_INST_VALU — which includes a matrix
// instruction for its whole 32 cycles — is 81-86 % of the wave-resident time of a SIMD: matrix and vector instructions of the
// co-resident waves take turns, they do not overlap.  Per key tile and wave that is 512 cycles of MFMA + ~350 of VALU (three
// quarters of it the 32 exp2): at head_dim 64 the matrix pipe cannot be more than ~60 % busy, the kernel has it at 48 %.
// A form software-pipelined INSIDE a wave (S(t+1) MFMAs issued between the exps of tile t, PV(t) per 16-key chunk as soon
// as its P exists, fragment reads two MFMAs ahead, separate K / VT rings; 160 registers, three waves per SIMD) was built,
// verified and measured the same per-SIMD time (412 vs 412 us): removed again.  Packed fp32 (v_pk_fma_f32 for the scale,
// v_pk_add_f32 for the row sums: 31 instructions instead of 63) measured 5-7 % SLOWER (394 -> 414-421 us): not kept.
// NW waves of 32 queries share every K / VT tile: NW = 8 (256 queries per workgroup) stages each tile once for twice the
// queries of NW = 4 — half the global->LDS traffic per query — at the same 16 waves per CU (two workgroups of 48 KiB).
template <int NW, int DBG = 0>
__global__ __launch_bounds__(NW * 64, 4) void attn_bf16_dma_kernel(AttnParams p) {
    // 2 stages x (K tile + VT tile); the Q rows of waves 4..7 (NW = 8) arrive in a third region
    __shared__ __attribute__((aligned(16))) char smem[(NW == 8 ? 6 : 4) * ATT_TILE_BYTES];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hi = lane >> 5;
    const int l31 = lane & 31;
    // 1-D grid: the nq query tiles that share one (batch, head)'s K/VT rows meet in one XCD's L2 (xcd_tile_order)
    constexpr int QT = 32 * NW;                 // queries per workgroup
    const int nq = (p.Nq + QT - 1) / QT;
    const int nbh = p.B * p.H;
    int qt, bh;
    xcd_tile_order((int)blockIdx.x, nq, nbh, p.dGroup, p.dNq, qt, bh);
    const int b = (int)uc_div((unsigned)bh, p.dH), h = bh - b * p.H;
    const int q0 = qt * QT + wave * 32;
    if constexpr (DBG & 8) {    // experiment: static priority by (approximate) workgroup slot on the CU
        const unsigned slot = (blockIdx.x >> 8) & 3u;
        if (slot == 0) __builtin_amdgcn_s_setprio(0);
        else if (slot == 1) __builtin_amdgcn_s_setprio(1);
        else if (slot == 2) __builtin_amdgcn_s_setprio(2);
        else __builtin_amdgcn_s_setprio(3);
    }
    if constexpr (DBG & 16) {   // experiment: de-phase the first round of workgroups by a quarter of a key tile each
        if (blockIdx.x < 1024u) {
            const unsigned slot = (blockIdx.x >> 8) & 3u;
            const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
            while (__builtin_amdgcn_s_memrealtime() - t0 < (unsigned long long)slot * 15u) __builtin_amdgcn_s_sleep(4);
        }
    }

    const bf16_t* Qb = (const bf16_t*)p.Q + (int64_t)b * p.q_sb + (int64_t)h * p.q_sh;
    const bf16_t* Kb = (const bf16_t*)p.K + (int64_t)b * p.k_sb + (int64_t)h * p.k_sh;
    const bf16_t* VTb = (const bf16_t*)p.V + ((int64_t)b * p.H + h) * 64 * (int64_t)p.npad;

    // ---- DMA assignment: a tile is 8 instructions of 8 rows x 128 B; wave w issues instructions PW*w .. PW*w + PW - 1 of both tiles ----
    constexpr int PW = 8 / NW;                  // 2 (four waves) or 1 (eight waves)
    uint4_t srd_k = make_srd(Kb);
    srd_k.z = (unsigned)__builtin_amdgcn_readfirstlane((int)((((int64_t)p.Nk - 1) * p.k_sn + 64) * 2));   // key rows >= Nk read as zeros
    const uint4_t srd_v = make_srd(VTb);
    const unsigned lds0 = lds_addr(smem);
    unsigned voff_k[PW], voff_v[PW];
#pragma unroll
    for (int i = 0; i < PW; ++i) {
        const int rr = (wave * PW + i) * 8 + (lane >> 3);
        const int cch = (lane & 7) ^ ((rr >> 1) & 7);         // logical chunk stored at physical chunk lane&7 of row rr
        voff_k[i] = (unsigned)(((int64_t)rr * p.k_sn + cch * 8) * 2);
        voff_v[i] = (unsigned)(((int64_t)rr * p.npad + cch * 8) * 2);
    }
    const unsigned kstep = (unsigned)(ATT_KV_TILE * p.k_sn * 2);   // bytes between key tiles of K
    auto issue_tile = [&](int t, int buf) {
        const unsigned dst = lds0 + (unsigned)(buf * 2 * ATT_TILE_BYTES + wave * (PW * 1024));
#pragma unroll
        for (int i = 0; i < PW; ++i) {
            dma16_buf_to_lds(voff_k[i], srd_k, (unsigned)t * kstep, __builtin_amdgcn_readfirstlane(dst + i * 1024));
            dma16_buf_to_lds(voff_v[i], srd_v, (unsigned)t * (ATT_KV_TILE * 2), __builtin_amdgcn_readfirstlane(dst + ATT_TILE_BYTES + i * 1024));
        }
    };

    // ---- Q: the wave's 32 query rows arrive by DMA too, into the second stage buffer, which the K/VT ring only needs from tile 1 on ----
    //      (waves 4..7 land behind it)
    att_q_rows_to_lds(Qb + (int64_t)q0 * p.q_sn, p.q_sn, (int64_t)p.Nq - q0, lds0 + (unsigned)(2 * ATT_TILE_BYTES + wave * 4096), lane);
    int r_off[4];   // fragment read offsets (K and VT tiles alike)
    att_frag_offsets(r_off, l31, hi);

    issue_tile(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // Q^T fragments (B operand): lane (q = l31, hi) holds Q[q][16s + 8hi .. +7], s = 0..3
    bf16x8_t qf[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) qf[s] = *reinterpret_cast<const bf16x8_t*>(smem + 2 * ATT_TILE_BYTES + wave * 4096 + r_off[s]);
    __syncthreads();     // every wave holds its Q fragments before tile 1 overwrites the buffer

    float16_t o[2];
    o[0] = (float16_t)(0.f);
    o[1] = (float16_t)(0.f);
    float m_run = ATT_MASKED;
    float l_run = 0.f;
    const float c = p.scale * ATT_LOG2E;  // scale * log2(e)
    if constexpr (NW == 8) {
        // static priority for the second-dispatched half (MI355X_MICROARCH.md "Two waves per SIMD", item 4): one s_setprio before the
        // loop, no per-segment flips (`wave` is a readfirstlane value: the branch is scalar, s_setprio ignores EXEC)
        if (p.prio_young && wave >= 4) __builtin_amdgcn_s_setprio(1);
    }

    const int nt = (p.Nk + ATT_KV_TILE - 1) / ATT_KV_TILE;
    for (int t = 0; t < nt; ++t) {
        const int buf = t & 1;
        if (t + 1 < nt) issue_tile(t + 1, buf ^ 1);
        const char* sk = smem + buf * 2 * ATT_TILE_BYTES;
        const char* sv = sk + ATT_TILE_BYTES;

        // The tile step and the LSE line below are written out, not taken from attention_tile.h: through its helpers (any of them, the
        // two MFMA loops included) the scheduler orders this loop differently, +1 % on whole tiles (profiles/attention_tile_codegen.txt)
        float16_t s[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            s[kb] = (float16_t)(0.f);
#pragma unroll
            for (int st = 0; st < 4; ++st) {
                const bf16x8_t kf = *reinterpret_cast<const bf16x8_t*>(sk + r_off[st] + kb * (32 * 128));
                s[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[st], s[kb], 0, 0, 0);
            }
        }
        if (t == nt - 1 && (p.Nk & (ATT_KV_TILE - 1))) {    // ragged last tile: keys >= Nk (zero K rows, zero VT pads) leave the softmax
            const int k0 = t * ATT_KV_TILE;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (k0 + kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi >= p.Nk) s[kb][r] = ATT_MASKED;   // key k0 + att_frag_row(kb, r, hi)
        }
        float mt = s[0][0];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) mt = fmaxf(mt, s[kb][r]);
        mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
        const bool grow = (mt - m_run) * c > 8.0f;     // deferred rescale, see attn_bf16_kernel
        if (__any(grow)) {
            const float m_new = fmaxf(m_run, mt);
            const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * c);
            m_run = m_new;
            l_run *= alpha;
#pragma unroll
            for (int db = 0; db < 2; ++db)
#pragma unroll
                for (int r = 0; r < 16; ++r) o[db][r] *= alpha;
        }
        const float mc = m_run * c;
        float psum = 0.f;
        bf16x8_t pf[4];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                float e[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    e[j] = (DBG & 2) ? s[kb][hf * 8 + j] : __builtin_amdgcn_exp2f(fmaf(s[kb][hf * 8 + j], c, -mc));
                    psum += e[j];
                }
                union { bf16x8_t v; unsigned u[4]; } pk;
#pragma unroll
                for (int j = 0; j < 4; ++j) pk.u[j] = pack_bf16x2(e[2 * j], e[2 * j + 1]);
                pf[kb * 2 + hf] = pk.v;
            }
        }
        l_run += psum;
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const bf16x8_t vf = *reinterpret_cast<const bf16x8_t*>(sv + r_off[g] + db * (32 * 128));
                if constexpr (!(DBG & 4)) o[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf[g], o[db], 0, 0, 0);
                else o[db][g] += (float)vf[0] * (float)pf[g][0];
            }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's pieces of tile t+1 have landed
        if constexpr (!(DBG & 1)) __syncthreads();                    // ... everyone's; and every wave is done reading tile t
    }

    // ---- normalise and store through the wave's private 4 KiB of the (now free) ring ----
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    const float inv = __builtin_amdgcn_rcpf(l_tot);
    const int q = q0 + l31;
    if (p.lse && q < p.Nq && hi == 0) p.lse[((int64_t)b * p.H + h) * p.Nq + q] = m_run * p.scale + logf(l_tot);
    att_store_rows_bounced(o, inv, smem + wave * 4096, (bf16_t*)p.O + (int64_t)b * p.o_sb + (int64_t)h * p.o_sh, p.o_sn, q0, p.Nq, lane);
}

// ---------------------------------------------------------------------------------------
// attn_bf16_rs_kernel — the same arithmetic as attn_bf16_dma_kernel<8>, ROLE-SPLIT (round 3): the loop is cut into segments that
// are either matrix work (PV of the previous key tile + QK^T of the next one: 16 MFMAs and their fragment reads) or vector work
// (the softmax of one tile: max, exp2, sums, conversions), every segment ends in a workgroup barrier, and the two halves of the
// workgroup run the SAME segment sequence one segment apart — while waves 0-3 are in a matrix segment, waves 4-7 (their partners
// on the four SIMDs: a workgroup's waves go to the SIMDs cyclically) are in a vector segment, and vice versa.
//
// Why: with every wave of a workgroup in the same phase (one barrier per tile), the matrix pipe of a SIMD sees both of its waves'
// MFMAs together and then neither — round 2 measured the exp2 work (-18 %) and the PV products (-20 %) as ADDITIVE costs and the
// pipe 41-48 % busy.  Here a SIMD's two waves of a workgroup alternate by construction (MI355X_MICROARCH.md "Two waves per SIMD":
// the pairing that nets is matrix beside vector); per tile and wave the matrix segment is 512 cycles and the vector segment ~350.
//
// Segment s = 0 .. 2 nt + 1 (nt key tiles); half h (0: waves 0-3, 1: waves 4-7) executes local segment ls = s - h:
//     ls = 2 t      matrix:  O += V(t-1) P(t-1)   (t >= 1),   S = K(t) Q^T   (t < nt)
//     ls = 2 t + 1  vector:  softmax of tile t: running max (deferred rescale), P(t) = exp2(..) as bf16 fragments, row sums
// LDS ring as before (two K buffers, two VT buffers): K(t) is read in segments 2t, 2t+1 and VT(t) in 2t+2, 2t+3; K(t+1) and VT(t)
// are issued at the start of segment 2t (their buffers were last read in segment 2t-1) and waited for before the barrier that
// ends segment 2t+1.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(512, 4) void attn_bf16_rs_kernel(AttnParams p) {
    constexpr int NW = 8;
    __shared__ __attribute__((aligned(16))) char smem[6 * ATT_TILE_BYTES];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = wave >> 2;
    const int hi = lane >> 5;
    const int l31 = lane & 31;
    constexpr int QT = 32 * NW;
    const int nq = (p.Nq + QT - 1) / QT;
    const int nbh = p.B * p.H;
    int qt, bh;
    xcd_tile_order((int)blockIdx.x, nq, nbh, p.dGroup, p.dNq, qt, bh);
    const int b = (int)uc_div((unsigned)bh, p.dH), h = bh - b * p.H;
    const int q0 = qt * QT + wave * 32;

    const bf16_t* Qb = (const bf16_t*)p.Q + (int64_t)b * p.q_sb + (int64_t)h * p.q_sh;
    const bf16_t* Kb = (const bf16_t*)p.K + (int64_t)b * p.k_sb + (int64_t)h * p.k_sh;
    const bf16_t* VTb = (const bf16_t*)p.V + ((int64_t)b * p.H + h) * 64 * (int64_t)p.npad;

    // DMA: a tile is 8 instructions of 8 rows x 128 B; wave w issues instruction w of the K tile and of the VT tile
    uint4_t srd_k = make_srd(Kb);
    srd_k.z = (unsigned)__builtin_amdgcn_readfirstlane((int)((((int64_t)p.Nk - 1) * p.k_sn + 64) * 2));   // key rows >= Nk read as zeros
    const uint4_t srd_v = make_srd(VTb);
    const unsigned lds0 = lds_addr(smem);
    unsigned voff_k, voff_v;
    {
        const int rr = wave * 8 + (lane >> 3);
        const int cch = (lane & 7) ^ ((rr >> 1) & 7);
        voff_k = (unsigned)(((int64_t)rr * p.k_sn + cch * 8) * 2);
        voff_v = (unsigned)(((int64_t)rr * p.npad + cch * 8) * 2);
    }
    const unsigned kstep = (unsigned)(ATT_KV_TILE * p.k_sn * 2);
    auto issue_k = [&](int t) {
        dma16_buf_to_lds(voff_k, srd_k, (unsigned)t * kstep, __builtin_amdgcn_readfirstlane(lds0 + (unsigned)((t & 1) * 2 * ATT_TILE_BYTES + wave * 1024)));
    };
    auto issue_v = [&](int t) {
        dma16_buf_to_lds(voff_v, srd_v, (unsigned)t * (ATT_KV_TILE * 2),
                  __builtin_amdgcn_readfirstlane(lds0 + (unsigned)((t & 1) * 2 * ATT_TILE_BYTES + ATT_TILE_BYTES + wave * 1024)));
    };
    // Q rows of this wave into the second stage (waves 0-3) / the third region (waves 4-7)
    att_q_rows_to_lds(Qb + (int64_t)q0 * p.q_sn, p.q_sn, (int64_t)p.Nq - q0, lds0 + (unsigned)(2 * ATT_TILE_BYTES + wave * 4096), lane);
    int r_off[4];
    att_frag_offsets(r_off, l31, hi);

    issue_k(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    bf16x8_t qf[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) qf[s] = *reinterpret_cast<const bf16x8_t*>(smem + 2 * ATT_TILE_BYTES + wave * 4096 + r_off[s]);
    __syncthreads();     // every wave holds its Q fragments before K(1) / VT(1) overwrite the buffer

    float16_t o[2], sc[2];
    o[0] = (float16_t)(0.f);
    o[1] = (float16_t)(0.f);
    sc[0] = (float16_t)(0.f);
    sc[1] = (float16_t)(0.f);
    AttProbsBf16 pr;
#pragma unroll
    for (int g = 0; g < 4; ++g) pr.pf[g] = (bf16x8_t)(0.f);
    float m_run = ATT_MASKED;
    float l_run = 0.f;
    const float c = p.scale * ATT_LOG2E;
    const int nt = (p.Nk + ATT_KV_TILE - 1) / ATT_KV_TILE;
    auto issue = [&](int t) __attribute__((always_inline)) {       // start of even segment 2t: VT(t) and K(t+1) set out
        if (t < nt) issue_v(t);
        if (t + 1 < nt) issue_k(t + 1);
    };
    auto matrix = [&](int t) __attribute__((always_inline)) {      // O += VT(t-1) P(t-1); S = K(t) Q^T
        if (t >= 1) att_pv_bf16(o, smem + ((t - 1) & 1) * 2 * ATT_TILE_BYTES + ATT_TILE_BYTES, r_off, pr.pf);
        if (t < nt) att_scores_bf16(sc, smem + (t & 1) * 2 * ATT_TILE_BYTES, r_off, qf);
    };
    auto vector = [&](int t) __attribute__((always_inline)) {      // softmax of tile t: sc -> pf
        if (t == nt - 1 && (p.Nk & (ATT_KV_TILE - 1))) {    // att_mask_tail as branches on a copy: with the shared select form this kernel spills 22 VGPRs
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                float16_t v = sc[kb];
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (t * ATT_KV_TILE + att_frag_row(kb, r, hi) >= p.Nk) v[r] = ATT_MASKED;
                sc[kb] = v;
            }
        }
        att_softmax_step(sc, m_run, l_run, o, c, pr);      // (the deferred rescale finds PV of tile t-1 complete)
    };
    // two loops with the same barrier sequence (2 nt + 2 segments), one segment apart: a single loop with a role switch keeps the
    // union of both roles' registers alive across its back edge (468 bytes of scratch at the 128-register budget)
    const bool seg_prio = p.prio_young == 2;     // experiment: priority 1 while in a matrix segment (cdna guide T5)
    if (half == 0) {
        for (int t = 0; t <= nt; ++t) {
            issue(t);
            if (seg_prio) __builtin_amdgcn_s_setprio(1);
            matrix(t);                                            // segment 2t
            if (seg_prio) __builtin_amdgcn_s_setprio(0);
            __syncthreads();
            if (t < nt) vector(t);                                // segment 2t + 1
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // what was issued at the start of segment 2t has landed
            __syncthreads();
        }
    } else {
        for (int t = 0; t <= nt; ++t) {
            issue(t);
            if (t >= 1) vector(t - 1);                            // segment 2t
            __syncthreads();
            if (seg_prio) __builtin_amdgcn_s_setprio(1);
            matrix(t);                                            // segment 2t + 1
            if (seg_prio) __builtin_amdgcn_s_setprio(0);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }
    }

    // ---- normalise and store through the wave's private 4 KiB of the (now free) ring ----
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    att_store_lse(p.lse, (int64_t)b * p.H + h, p.Nq, q0 + l31, hi, m_run, p.scale, l_tot);
    att_store_rows_bounced(o, __builtin_amdgcn_rcpf(l_tot), smem + wave * 4096, (bf16_t*)p.O + (int64_t)b * p.o_sb + (int64_t)h * p.o_sh, p.o_sn, q0, p.Nq, lane);
}

// ---------------------------------------------------------------------------------------
// row-major V -> VT packing (for callers that did not get VT from the GEMM epilogue)
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void vt_pack_kernel(const bf16_t* __restrict__ V, bf16_t* __restrict__ VT, int H,
                                                      int Nk, int D, int npad, int64_t v_sb, int64_t v_sn,
                                                      int64_t v_sh) {
    // block: (key tile of 64, head, batch); LDS transpose of a [64 keys][D] tile
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    bf16_t* tile = reinterpret_cast<bf16_t*>(smem_raw);  // [64][D+2]
    const int b = blockIdx.z, h = blockIdx.y, k0 = blockIdx.x * 64;
    const int ld = D + 2;
    const bf16_t* vb = V + (int64_t)b * v_sb + (int64_t)h * v_sh;
    for (int idx = threadIdx.x; idx < 64 * D; idx += blockDim.x) {
        const int key = idx / D, d = idx % D;
        tile[key * ld + d] = (k0 + key < Nk) ? vb[(int64_t)(k0 + key) * v_sn + d] : (bf16_t)0;
    }
    __syncthreads();
    bf16_t* out = VT + ((int64_t)b * H + h) * D * (int64_t)npad + k0;
    for (int idx = threadIdx.x; idx < 64 * D; idx += blockDim.x) {
        const int pos = idx & 63, d = idx >> 6;
        const int key = (pos & ~15) + vt_key_of_pos(pos & 15);
        out[(int64_t)d * npad + pos] = tile[key * ld + d];
    }
}

// D == 64, 16-byte accesses on both sides: 8-channel chunks in, 8-position chunks out (the generic kernel above moves single
// bf16 values and divides per element)
__global__ __launch_bounds__(256) void vt_pack64_kernel(const bf16_t* __restrict__ V, bf16_t* __restrict__ VT, int H, int Nk,
                                                        int npad, int64_t v_sb, int64_t v_sn, int64_t v_sh) {
    __shared__ __attribute__((aligned(16))) bf16_t tile[64][64 + 8];   // [key][d], 144-byte rows
    const int b = blockIdx.z, h = blockIdx.y, k0 = blockIdx.x * 64;
    const bf16_t* vb = V + (int64_t)b * v_sb + (int64_t)h * v_sh;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int idx = threadIdx.x + it * 256;          // 512 chunks: key = idx >> 3, 8 channels from (idx & 7) * 8
        const int key = idx >> 3, c8 = idx & 7;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (k0 + key < Nk) v = *reinterpret_cast<const uint4*>(vb + (int64_t)(k0 + key) * v_sn + c8 * 8);
        *reinterpret_cast<uint4*>(&tile[key][c8 * 8]) = v;
    }
    __syncthreads();
    bf16_t* out = VT + ((int64_t)b * H + h) * 64 * (int64_t)npad + k0;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int idx = threadIdx.x + it * 256;          // 512 chunks: channel d = idx >> 3, positions (idx & 7) * 8 .. +7
        const int d = idx >> 3, p8 = (idx & 7) * 8;
        unsigned short e[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int pos = p8 + j;
            e[j] = tile[(pos & ~15) + vt_key_of_pos(pos & 15)][d];
        }
        uint4 o;
        o.x = (unsigned)e[0] | ((unsigned)e[1] << 16); o.y = (unsigned)e[2] | ((unsigned)e[3] << 16);
        o.z = (unsigned)e[4] | ((unsigned)e[5] << 16); o.w = (unsigned)e[6] | ((unsigned)e[7] << 16);
        *reinterpret_cast<uint4*>(out + (int64_t)d * npad + p8) = o;
    }
}

extern "C" int uc_vt_pack(const void* V, void* VT, int B, int H, int Nk, int D, int64_t v_sb, int64_t v_sn,
                          int64_t v_sh, uc_stream_t stream) {
    UC_REQUIRE(V && VT, "uc_vt_pack: null pointer");
    UC_REQUIRE(B > 0 && H > 0 && Nk > 0 && D > 0 && D <= 256, "uc_vt_pack: bad shape");
    const int npad = (Nk + 63) / 64 * 64;
    if (D == 64 && v_sb % 8 == 0 && v_sn % 8 == 0 && v_sh % 8 == 0 && (uintptr_t)V % 16 == 0 && (uintptr_t)VT % 16 == 0)
        hipLaunchKernelGGL(vt_pack64_kernel, dim3(npad / 64, H, B), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)V, (bf16_t*)VT, H, Nk,
                           npad, v_sb, v_sn, v_sh);
    else
        hipLaunchKernelGGL(vt_pack_kernel, dim3(npad / 64, H, B), dim3(256), (size_t)64 * (D + 2) * 2, (hipStream_t)stream,
                           (const bf16_t*)V, (bf16_t*)VT, H, Nk, D, npad, v_sb, v_sn, v_sh);
    UC_CHECK_LAUNCH("uc_vt_pack");
    return UC_OK;
}

// ---------------------------------------------------------------------------------------
// fp32 verification kernel: one thread per query, 32-key tiles of K and V in LDS (broadcast reads)
// ---------------------------------------------------------------------------------------
#define F32_KT 32

template <int DMAX, bool DROP = false>
__global__ __launch_bounds__(128) void attn_f32_kernel(AttnParams p) {
    __shared__ float Ks[F32_KT][DMAX];
    __shared__ float Vs[F32_KT][DMAX];
    const int b = blockIdx.z, h = blockIdx.y;
    const int q = blockIdx.x * 128 + threadIdx.x;
    const int D = p.D;
    const float* Qb = (const float*)p.Q + (int64_t)b * p.q_sb + (int64_t)h * p.q_sh;
    const float* Kb = (const float*)p.K + (int64_t)b * p.k_sb + (int64_t)h * p.k_sh;
    const float* Vb = (const float*)p.V + (int64_t)b * p.v_sb + (int64_t)h * p.v_sh;
    const bool active = q < p.Nq;
    float qr[DMAX], acc[DMAX];
#pragma unroll
    for (int d = 0; d < DMAX; ++d) {
        qr[d] = (active && d < D) ? Qb[(int64_t)q * p.q_sn + d] : 0.f;
        acc[d] = 0.f;
    }
    float m_run = -INFINITY, l_run = 0.f;
    unsigned dk1 = 0, dk2 = 0;
    if constexpr (DROP) uc_drop_keys(p.drop, (unsigned)(b * p.H + h), dk1, dk2);
    for (int k0 = 0; k0 < p.Nk; k0 += F32_KT) {
        __syncthreads();
        for (int idx = threadIdx.x; idx < F32_KT * DMAX; idx += blockDim.x) {
            const int kk = idx / DMAX, d = idx % DMAX;
            const bool ok = (k0 + kk < p.Nk) && d < D;
            Ks[kk][d] = ok ? Kb[(int64_t)(k0 + kk) * p.k_sn + d] : 0.f;
            Vs[kk][d] = ok ? Vb[(int64_t)(k0 + kk) * p.v_sn + d] : 0.f;
        }
        __syncthreads();
        float s[F32_KT];
        float mt = -INFINITY;
#pragma unroll
        for (int kk = 0; kk < F32_KT; ++kk) {
            float a = 0.f;
#pragma unroll
            for (int d = 0; d < DMAX; ++d) a = fmaf(qr[d], Ks[kk][d], a);
            a *= p.scale;
            s[kk] = (k0 + kk < p.Nk) ? a : -INFINITY;
            mt = fmaxf(mt, s[kk]);
        }
        const float m_new = fmaxf(m_run, mt);
        const float alpha = (m_run == -INFINITY) ? 0.f : expf(m_run - m_new);
        l_run *= alpha;
#pragma unroll
        for (int d = 0; d < DMAX; ++d) acc[d] *= alpha;
#pragma unroll
        for (int kk = 0; kk < F32_KT; ++kk) {
            float pw = (k0 + kk < p.Nk) ? expf(s[kk] - m_new) : 0.f;
            l_run += pw;
            if constexpr (DROP) pw = uc_drop_hash(dk1, dk2, (unsigned)q, (unsigned)(k0 + kk)) >= p.drop.thr ? pw * p.drop.keep_scale : 0.f;
#pragma unroll
            for (int d = 0; d < DMAX; ++d) acc[d] = fmaf(pw, Vs[kk][d], acc[d]);
        }
        m_run = m_new;
    }
    if (active) {
        if (p.lse) p.lse[((int64_t)b * p.H + h) * p.Nq + q] = m_run + logf(l_run);
        float* op = (float*)p.O + (int64_t)b * p.o_sb + (int64_t)q * p.o_sn + (int64_t)h * p.o_sh;
        const float inv = 1.0f / l_run;
#pragma unroll
        for (int d = 0; d < DMAX; ++d)
            if (d < D) op[d] = acc[d] * inv;
    }
}

// keep mask of uc_attention_fwd / uc_attention_bwd with drop_p > 0 as bytes [B, H, Nq, Nk] (1 = kept): what a reference implementation
// multiplies the probabilities with (tests), evaluated by the same function as the kernels
__global__ void attn_drop_mask_kernel(unsigned char* mask, int H, int Nq, int Nk, int64_t total, UcDropout d) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int k = (int)(idx % Nk);
    const int q = (int)((idx / Nk) % Nq);
    const unsigned bh = (unsigned)(idx / ((int64_t)Nk * Nq));
    unsigned k1, k2;
    uc_drop_keys(d, bh, k1, k2);
    mask[idx] = uc_drop_hash(k1, k2, (unsigned)q, (unsigned)k) >= d.thr ? 1 : 0;
}

extern "C" int uc_attention_drop_mask(void* mask, int B, int H, int Nq, int Nk, float drop_p, unsigned long long seed, uc_stream_t stream) {
    UC_REQUIRE(mask && B > 0 && H > 0 && Nq > 0 && Nk > 0, "uc_attention_drop_mask: bad arguments");
    UC_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "uc_attention_drop_mask: drop_p must be in [0, 1) (got %g)", (double)drop_p);
    const int64_t total = (int64_t)B * H * Nq * Nk;
    hipLaunchKernelGGL(attn_drop_mask_kernel, dim3((unsigned)ceil_div64(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       (unsigned char*)mask, H, Nq, Nk, total, uc_make_dropout(drop_p, seed));
    UC_CHECK_LAUNCH("uc_attention_drop_mask");
    return UC_OK;
}

#ifdef UC_DIAG
// diag build: the four-wave DMA kernel with its anatomy switches (results are wrong): 1 no per-tile barrier, 2 no exp (P = S),
// 4 no PV MFMAs
static void launch_attn_dma4_dbg(int dbg, dim3 grid, hipStream_t st, const AttnParams& p) {
    if (dbg == 1) hipLaunchKernelGGL((attn_bf16_dma_kernel<4, 1>), grid, dim3(256), 0, st, p);
    else if (dbg == 2) hipLaunchKernelGGL((attn_bf16_dma_kernel<4, 2>), grid, dim3(256), 0, st, p);
    else if (dbg == 3) hipLaunchKernelGGL((attn_bf16_dma_kernel<4, 3>), grid, dim3(256), 0, st, p);
    else if (dbg == 4) hipLaunchKernelGGL((attn_bf16_dma_kernel<4, 4>), grid, dim3(256), 0, st, p);
    else if (dbg == 5) hipLaunchKernelGGL((attn_bf16_dma_kernel<4, 5>), grid, dim3(256), 0, st, p);
    else if (dbg == 8) hipLaunchKernelGGL((attn_bf16_dma_kernel<4, 8>), grid, dim3(256), 0, st, p);
    else if (dbg == 16) hipLaunchKernelGGL((attn_bf16_dma_kernel<4, 16>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((attn_bf16_dma_kernel<4, 24>), grid, dim3(256), 0, st, p);
}
#endif

// what the kernels of a served forward need of the operands' layout: the bf16 kernels of every head_dim (16-byte row loads of Q / K,
// packed VT, 8-byte stores of O) alike, the fp32 ones a row-major V
static int attention_fwd_layout(const uc_attention_desc& d, const char* fn) {
    if (d.dtype == UC_F32) {
        UC_REQUIRE(d.v_layout == UC_V_ROWMAJOR, "%s(f32): V must be row-major", fn);
        return UC_OK;
    }
    UC_REQUIRE(d.v_layout == UC_V_PACKED_T, "%s(bf16): V must be in the packed VT layout (uc_vt_pack)", fn);
    UC_REQUIRE(d.q_sb % 8 == 0 && d.q_sn % 8 == 0 && d.q_sh % 8 == 0 && d.k_sb % 8 == 0 && d.k_sn % 8 == 0 && d.k_sh % 8 == 0,
               "%s(bf16): Q/K strides must be multiples of 8 elements", fn);
    UC_REQUIRE(d.o_sb % 4 == 0 && d.o_sn % 4 == 0 && d.o_sh % 4 == 0, "%s(bf16): O strides must be multiples of 4", fn);
    UC_REQUIRE(((uintptr_t)d.Q % 16 == 0) && ((uintptr_t)d.K % 16 == 0) && ((uintptr_t)d.V % 16 == 0) && ((uintptr_t)d.O % 8 == 0),
               "%s(bf16): pointer alignment", fn);
    return UC_OK;
}

// uc_attention_fwd: check the arguments, snapshot the knobs, plan the launch once (attention_plan.h: a refusal or a kernel with its
// grid), check the layout the served kernels need, fill AttnParams and carry the plan out
extern "C" int uc_attention_fwd(const uc_attention_desc* desc, uc_stream_t stream) {
    UC_REQUIRE(desc, "uc_attention_fwd: null descriptor");
    const uc_attention_desc& d = *desc;
    const char* fn = "uc_attention_fwd";
    const void *Q = d.Q, *K = d.K, *V = d.V;
    void* O = d.O;
    const int B = d.B, H = d.H, Nq = d.Nq, Nk = d.Nk, D = d.D;
    UC_REQUIRE(d.drop_p >= 0.f && d.drop_p < 1.f, "%s: drop_p must be in [0, 1) (got %g)", fn, (double)d.drop_p);
    const bool drop = d.drop_p != 0.f;
    UC_REQUIRE(Q && K && V && O, "%s: null pointer", fn);
    UC_REQUIRE(B > 0 && H > 0 && Nq > 0 && Nk > 0 && D > 0, "%s: bad shape", fn);
    UC_REQUIRE(H <= 65535 && B <= 65535, "%s: B and H must fit a grid dimension", fn);
    // the knob snapshot: uc_knobs() first (it stores the environment's initial values of the run-time switchable ones)
    const UcKnobs& kn = uc_knobs();
    AttnKnobs knobs = {};
    knobs.p64 = g_uc_attn_p64.load(std::memory_order_relaxed);
    knobs.role_split = g_uc_attn_rs.load(std::memory_order_relaxed);
    knobs.cus = uc_num_cus();
#ifdef UC_DIAG
    knobs.dbg = kn.attn_dbg;
#endif
    const AttnFwdPlan plan = uc_attention_fwd_plan(d, knobs);
    if (plan.refused) {
        uc_set_error(uc_attention_refusal_format(plan.refused), fn, plan.refused == UC_AR_DTYPE ? d.dtype : D);
        return UC_ERR_BAD_ARG;
    }
    if (const int bad = attention_fwd_layout(d, fn)) return bad;

    AttnParams p;
    p.Q = Q; p.K = K; p.V = V; p.O = O; p.B = B; p.H = H; p.Nq = Nq; p.Nk = Nk; p.D = D;
    p.q_sb = d.q_sb; p.q_sn = d.q_sn; p.q_sh = d.q_sh; p.k_sb = d.k_sb; p.k_sn = d.k_sn; p.k_sh = d.k_sh;
    p.v_sb = d.v_sb; p.v_sn = d.v_sn; p.v_sh = d.v_sh; p.o_sb = d.o_sb; p.o_sn = d.o_sn; p.o_sh = d.o_sh;
    p.npad = (Nk + 63) / 64 * 64;
    p.scale = d.scale;
    p.lse = d.lse;
    p.prio_young = drop ? 0 : kn.attn_prio;
    p.drop = uc_make_dropout(drop ? d.drop_p : 0.f, drop ? d.seed : 0ull);
    if (plan.nqt) { p.dGroup = uc_make_fastdiv((unsigned)(8 * plan.nqt)); p.dNq = uc_make_fastdiv((unsigned)plan.nqt); p.dH = uc_make_fastdiv((unsigned)H); }
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(plan.grid[0], plan.grid[1], plan.grid[2]), block(plan.block);
    switch (plan.kernel) {
        case UC_AF_REG128: hipLaunchKernelGGL(attn_bf16_kernel, grid, block, 0, st, p); break;
        case UC_AF_DMA4: hipLaunchKernelGGL(attn_bf16_dma_kernel<4>, grid, block, 0, st, p); break;
        case UC_AF_DMA8: hipLaunchKernelGGL(attn_bf16_dma_kernel<8>, grid, block, 0, st, p); break;
        case UC_AF_RS8: hipLaunchKernelGGL(attn_bf16_rs_kernel, grid, block, 0, st, p); break;
        case UC_AF_P64:
        case UC_AF_P64_TAIL: {
            AttnP64Params pp;
            pp.Q = Q; pp.K = K; pp.V = V; pp.O = O; pp.lse = d.lse; pp.B = B; pp.H = H; pp.Nq = Nq; pp.Nk = Nk;
            pp.q_sb = d.q_sb; pp.q_sn = d.q_sn; pp.q_sh = d.q_sh; pp.k_sb = d.k_sb; pp.k_sn = d.k_sn; pp.k_sh = d.k_sh;
            pp.o_sb = d.o_sb; pp.o_sn = d.o_sn; pp.o_sh = d.o_sh;
            pp.npad = p.npad; pp.c = d.scale * ATT_LOG2E; pp.q_prescaled = 0;
            pp.nq = (Nq + 255) / 256; pp.dNq = uc_make_fastdiv((unsigned)pp.nq); pp.dH = uc_make_fastdiv((unsigned)H);
            pp.dbg = nullptr;
            if (plan.kernel == UC_AF_P64_TAIL) hipLaunchKernelGGL(attn_bf16_p64_kernel<true>, grid, block, 0, st, pp);
            else hipLaunchKernelGGL(attn_bf16_p64_kernel<false>, grid, block, 0, st, pp);
            UC_CHECK_LAUNCH("uc_attention_fwd (persistent kernel)");
            hipLaunchKernelGGL(attn_bf16_fixup_kernel, dim3((unsigned)plan.fixup_grid), dim3(256), 0, st, p);
            break;
        }
        case UC_AF_REG128_DROP: hipLaunchKernelGGL(attn_bf16_drop_kernel, grid, block, 0, st, p); break;
        case UC_AF_F32_32: hipLaunchKernelGGL((attn_f32_kernel<32>), grid, block, 0, st, p); break;
        case UC_AF_F32_64: hipLaunchKernelGGL((attn_f32_kernel<64>), grid, block, 0, st, p); break;
        case UC_AF_F32_96: hipLaunchKernelGGL((attn_f32_kernel<96>), grid, block, 0, st, p); break;
        case UC_AF_F32_32_DROP: hipLaunchKernelGGL((attn_f32_kernel<32, true>), grid, block, 0, st, p); break;
        case UC_AF_F32_64_DROP: hipLaunchKernelGGL((attn_f32_kernel<64, true>), grid, block, 0, st, p); break;
        case UC_AF_BF16_80:
        case UC_AF_BF16_96: return uc_attention_wide_fwd_launch(d, plan, stream);   // (its kernels take AttnWideParams: attention_wide.hip)
        case UC_AF_DMA4_DBG:
#ifdef UC_DIAG
            launch_attn_dma4_dbg(plan.dbg, grid, st, p);
#endif
            break;
    }
    UC_CHECK_LAUNCH(fn);
    return UC_OK;
}

