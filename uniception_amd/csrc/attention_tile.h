// What the attention forward kernels that give each wave 32 queries share (attention.hip, attention_fp8.hip, attention_x3.hip,
// attention_diff.hip): the per-key-tile step and the pieces around it.  Each of them exists ONCE, here.  Device-only.
//
// The layout all of them compute in (head_dim 64, v_mfma_f32_32x32x16_bf16 or its e4m3 K=64 sibling):
//   A wave owns 32 queries of one (batch, head).  Per 64-key tile:   S^T[key,q] = K . Q^T   (A = K rows from LDS, B = Q^T held in
//   registers).  The swapped product puts a query's whole score column in ONE lane pair (lane, lane^32): row max / row sum are 31
//   in-register ops + one cross-half exchange; the running max, the rescale factor and the normaliser are lane-local scalars.
//   P^T (bf16) in the S^T accumulator layout is directly the B operand of  O^T[d,q] += V^T . P^T  when the key order inside each
//   16-key group is permuted the same way on the V side — which is what the "VT" layout (uc_hip.h) bakes into memory, so the A
//   operand V^T[d, 8 keys] is one 16-byte LDS read.  K and VT tiles live in LDS as XOR-swizzled 128-byte rows (tile_swz), two stages.
//   Lane (l31 = lane & 31, hi = lane >> 5) holds query l31; which keys (scores) and channels (outputs) its accumulator registers
//   hold is att_frag_row below.
#pragma once
#include "mma_tile.h"

constexpr int ATT_KV_TILE = 64;                         // keys per tile
constexpr int ATT_TILE_BYTES = ATT_KV_TILE * 128;       // one bf16 tile: 64 rows x 128 B (64 keys x 64 channels, or 64 channels x 64 key positions)
constexpr float ATT_LOG2E = 1.44269504088896340736f;    // scores are scaled by scale * log2(e): every exponential is an exp2
constexpr float ATT_LN2 = 0.69314718055994530942f;
constexpr float ATT_MASKED = -1e30f;                    // score of a key that does not exist; the running max starts there too

// THE fragment map of a 32x32 accumulator block: register r (0..15) of block blk in lane half hi is row 32 blk + (r&3) + 8 (r>>2)
// + 4 hi — the KEY of a score block (S^T), the CHANNEL of an output block (O^T).  The column is the query l31.
__device__ __forceinline__ constexpr int att_frag_row(int blk, int r, int hi) { return 32 * blk + (r & 3) + 8 * (r >> 2) + 4 * hi; }

// fragment read offsets into a swizzled tile: row l31 (+32 per block, an immediate: rows r and r+32 share the swizzle key), chunk 2 st + hi
__device__ __forceinline__ void att_frag_offsets(int (&r_off)[4], const int l31, const int hi) {
#pragma unroll
    for (int st = 0; st < 4; ++st) r_off[st] = tile_swz(l31, 2 * st + hi);
}

// ---- S^T = K . Q^T : two 32-key blocks, 4 k-steps (16 channels) each (bf16 32x32x16 form) ----
__device__ __forceinline__ void att_scores_bf16(float16_t (&s)[2], const char* sk, const int (&r_off)[4], const bf16x8_t (&qf)[4]) {
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
        s[kb] = (float16_t)(0.f);
#pragma unroll
        for (int st = 0; st < 4; ++st) {
            const bf16x8_t kf = *reinterpret_cast<const bf16x8_t*>(sk + r_off[st] + kb * (32 * 128));
            s[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[st], s[kb], 0, 0, 0);
        }
    }
}
// ---- O^T += V^T . P^T : two 32-channel blocks x four 16-key slabs ----
__device__ __forceinline__ void att_pv_bf16(float16_t (&o)[2], const char* sv, const int (&r_off)[4], const bf16x8_t (&pf)[4]) {
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const bf16x8_t vf = *reinterpret_cast<const bf16x8_t*>(sv + r_off[g] + db * (32 * 128));
            o[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf[g], o[db], 0, 0, 0);
        }
}

// Ragged last tile (keys from k0): the scores of keys >= Nk leave the softmax.  Call it under a WAVE-UNIFORM guard that is false on
// every whole tile (k0 + ATT_KV_TILE > Nk, or t == nt - 1 && (Nk & 63)): whole tiles branch over these 32 selects.
__device__ __forceinline__ void att_mask_tail(float16_t (&s)[2], const int k0, const int Nk, const int hi) {
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) s[kb][r] = k0 + att_frag_row(kb, r, hi) >= Nk ? ATT_MASKED : s[kb][r];
}

// ---------------------------------------------------------------------------------------------------------------------------
// Probability emission policies of att_softmax_step: how the 64 probabilities of a lane become the B operand(s) of the PV product.
// GROUP consecutive accumulator registers are handed to put() at a time; RESCALE_LOG2 is the deferred-rescale threshold (P stays
// <= 2^RESCALE_LOG2); EXP2_DOMAIN: the scores already carry scale * log2(e).
// ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bf16x8_t att_pack_bf16x8(const float (&e)[8]) {
    union { bf16x8_t v; unsigned u[4]; } pk;
#pragma unroll
    for (int j = 0; j < 4; ++j) pk.u[j] = pack_bf16x2(e[2 * j], e[2 * j + 1]);
    return pk.v;
}
// plain bf16: P^T B-operand fragments, slab g = 2*kb + half, 8 key slots per lane
struct AttProbsBf16 {
    static constexpr int GROUP = 8;
    static constexpr float RESCALE_LOG2 = 8.0f;
    static constexpr bool EXP2_DOMAIN = false;
    bf16x8_t pf[4];
    __device__ __forceinline__ void put(const int kb, const int g, const float (&e)[8]) { pf[kb * 2 + g] = att_pack_bf16x8(e); }
};
// bf16 with attention dropout: the row sum — the softmax's normalisation — takes every probability, the P^T operand only the kept
// ones, scaled by 1 / (1 - p).  (k1, k2) = uc_drop_keys of the (batch, head), q the lane's query, k0 the tile's first key.
struct AttProbsBf16Drop {
    static constexpr int GROUP = 8;
    static constexpr float RESCALE_LOG2 = 8.0f;
    static constexpr bool EXP2_DOMAIN = false;
    bf16x8_t pf[4];
    unsigned k1, k2, q;
    int k0, hi;
    UcDropout drop;
    __device__ __forceinline__ void put(const int kb, const int g, const float (&e)[8]) {
        float kept[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const unsigned key = (unsigned)(k0 + att_frag_row(kb, g * 8 + j, hi));
            kept[j] = uc_drop_hash(k1, k2, q, key) >= drop.thr ? e[j] * drop.keep_scale : 0.f;
        }
        pf[kb * 2 + g] = att_pack_bf16x8(kept);
    }
};
// bf16 hi / lo split (P = ph + pl to ~2^-16 relative), scores in the exp2 domain
struct AttProbsBf16x3 {
    static constexpr int GROUP = 8;
    static constexpr float RESCALE_LOG2 = 8.0f;   // the split is floating point: its RELATIVE accuracy does not depend on the scale of P
    static constexpr bool EXP2_DOMAIN = true;
    bf16x8_t ph[4], pl[4];
    __device__ __forceinline__ void put(const int kb, const int g, const float (&e)[8]) {
        union { bf16x8_t v; unsigned u[4]; } a, c;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            a.u[j] = pack_bf16x2(e[2 * j], e[2 * j + 1]);
            c.u[j] = pack_bf16x2(e[2 * j] - __uint_as_float(a.u[j] << 16), e[2 * j + 1] - __uint_as_float(a.u[j] & 0xffff0000u));
        }
        ph[kb * 2 + g] = a.v;
        pl[kb * 2 + g] = c.v;
    }
};

// One online-softmax step of a lane pair's query over the 64 scores s[2][16] (keys k0 + att_frag_row(kb, r, hi), tail already masked):
// row maximum over the lane pair, deferred rescale of (m_run, l_run, o), then the probabilities — summed into l_run (lane-partial:
// the pair is added in the epilogue) and handed to the policy.  c = scale * log2(e) (unused in the exp2 domain).
// Deferred rescale: keep the old running max while no query of the wave grew by more than 2^RESCALE_LOG2 in the exp2 domain (P stays
// <= 2^RESCALE_LOG2: 2^8 for the bf16 emissions, 2^2 for e4m3; the factor cancels in the final O/l ratio); the O/l rescale then runs
// on a wave-uniform branch.
template <class Probs>
__device__ __forceinline__ void att_softmax_step(const float16_t (&s)[2], float& m_run, float& l_run, float16_t (&o)[2], const float c, Probs& pr) {
    float mt = s[0][0];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) mt = fmaxf(mt, s[kb][r]);
    mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
    const bool grow = Probs::EXP2_DOMAIN ? mt - m_run > Probs::RESCALE_LOG2 : (mt - m_run) * c > Probs::RESCALE_LOG2;
    if (__any(grow)) {
        const float m_new = fmaxf(m_run, mt);
        const float alpha = __builtin_amdgcn_exp2f(Probs::EXP2_DOMAIN ? m_run - m_new : (m_run - m_new) * c);
        m_run = m_new;
        l_run *= alpha;
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[db][r] *= alpha;
    }
    const float mc = m_run * c;
    float psum = 0.f;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
        for (int g = 0; g < 16 / Probs::GROUP; ++g) {
            float e[Probs::GROUP];
#pragma unroll
            for (int j = 0; j < Probs::GROUP; ++j) {
                const float sc = s[kb][g * Probs::GROUP + j];
                e[j] = __builtin_amdgcn_exp2f(Probs::EXP2_DOMAIN ? sc - m_run : fmaf(sc, c, -mc));
                psum += e[j];
            }
            pr.put(kb, g, e);
        }
    }
    l_run += psum;
}

// ---------------------------------------------------------------------------------------------------------------------------
// register-staged kernels: one 16-byte chunk of the VT tile (row = channel d, the 8 key positions [k0 + 8cc, +8)); on the tail
// tile the positions whose key is out of range are zeroed (probability 0 times anything, finite or not)
// ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint4 att_load_vt_chunk(const bf16_t* VTb, const int row, const int npad, const int k0, const int cc, const int Nk) {
    uint4 v = *reinterpret_cast<const uint4*>(VTb + (int64_t)row * npad + k0 + cc * 8);
    if (k0 + ATT_KV_TILE > Nk) {
        const int gbase = k0 + ((cc * 8) & ~15);
        const int pbase = (cc * 8) & 15;
        unsigned m[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (gbase + vt_key_of_pos(pbase + j) >= Nk) m[j >> 1] &= (j & 1) ? 0x0000ffffu : 0xffff0000u;
        v.x &= m[0]; v.y &= m[1]; v.z &= m[2]; v.w &= m[3];
    }
    return v;
}

// LDS-DMA kernels: the wave's 32 query rows (128 B each, row_stride elements apart, from q_rows0 = the first one) arrive by DMA too —
// 4 instructions of 8 whole rows instead of 4 loads that touch 32 rows x 32 B each (the vector memory path pays per row segment) —
// as a swizzled 4 KiB tile at LDS byte address dst.  The descriptor covers min(32, rows_left) rows: the rows beyond Nq read as zeros.
__device__ __forceinline__ void att_q_rows_to_lds(const bf16_t* q_row0, const int64_t row_stride, const int64_t rows_left, const unsigned dst, const int lane) {
    const int64_t q_rows = min((int64_t)32, rows_left);
    const uint4_t srd_q = make_srd(q_row0, q_rows > 0 ? (unsigned)(((q_rows - 1) * row_stride + 64) * 2) : 0u);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int rr = i * 8 + (lane >> 3);
        const int cch = (lane & 7) ^ ((rr >> 1) & 7);
        dma16_buf_to_lds((unsigned)(((int64_t)rr * row_stride + cch * 8) * 2), srd_q, 0u, __builtin_amdgcn_readfirstlane(dst + i * 1024));
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// epilogues.  l_tot = l_run + __shfl_xor(l_run, 32): the pair's row sum.
// ---------------------------------------------------------------------------------------------------------------------------
// log-sum-exp of the scaled scores of query q (saved for the backward): m_scale turns the running max into nats (the scale, or ln 2
// when the scores are in the exp2 domain)
__device__ __forceinline__ void att_store_lse(float* lse, const int64_t bh, const int Nq, const int q, const int hi, const float m_run, const float m_scale,
                                              const float l_tot) {
    if (lse && q < Nq && hi == 0) lse[bh * Nq + q] = m_run * m_scale + logf(l_tot);
}
// normalise and store directly: lane holds 4 consecutive channels per (db, r>>2); op = the row of query l31
__device__ __forceinline__ void att_store_rows_direct(const float16_t (&o)[2], const float inv, bf16_t* op, const int hi) {
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const int d = att_frag_row(db, g4 * 4, hi);
            uint2 pk;
            pk.x = pack_bf16x2(o[db][g4 * 4 + 0] * inv, o[db][g4 * 4 + 1] * inv);
            pk.y = pack_bf16x2(o[db][g4 * 4 + 2] * inv, o[db][g4 * 4 + 3] * inv);
            *reinterpret_cast<uint2*>(op + d) = pk;
        }
}
// normalise; bounce the wave's 32 x 64 outputs through its private 4 KiB of LDS (ob) so that every store instruction writes 8 whole
// 128-B rows instead of 32 rows x 16 B.  obase = row 0 of this (batch, head); rows q0 + R >= Nq are not stored.
__device__ __forceinline__ void att_store_rows_bounced(const float16_t (&o)[2], const float inv, char* ob, bf16_t* obase, const int64_t o_sn, const int q0,
                                                       const int Nq, const int lane) {
    const int hi = lane >> 5, l31 = lane & 31;
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            uint2 pk;       // channels att_frag_row(db, 4 g4, hi) .. +3 of query l31 = half of 16-B chunk 4db + g4
            pk.x = pack_bf16x2(o[db][g4 * 4 + 0] * inv, o[db][g4 * 4 + 1] * inv);
            pk.y = pack_bf16x2(o[db][g4 * 4 + 2] * inv, o[db][g4 * 4 + 3] * inv);
            *reinterpret_cast<uint2*>(ob + l31 * 128 + (((4 * db + g4) ^ (l31 & 7)) << 4) + hi * 8) = pk;
        }
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) {
        const int R = 8 * ps + (lane >> 3);
        const int chunk = (lane & 7) ^ (R & 7);
        const uint4 v = *reinterpret_cast<const uint4*>(ob + R * 128 + ((lane & 7) << 4));
        if (q0 + R < Nq) *reinterpret_cast<uint4*>(obase + (int64_t)(q0 + R) * o_sn + chunk * 8) = v;
    }
}
