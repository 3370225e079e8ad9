#pragma once
// Dense bf16 GEMM for gfx950 with direct global->LDS staging (LDS-DMA, mma_tile.h: 1 KiB per wave-instruction).
//
//   C[M,N] = epilogue(A[M,K] . W[N,K]^T),  K % 64 == 0, A/W bf16 row-major.
//
// Tile geometry: BM x BN x 64 per workgroup, every wavefront owns a 64x64 sub-tile (4x4 MFMA 16x16x32 fragments).
// LDS image of a stage: (BM + BN) rows x 128 B.  The DMA writes lane-linear (wave base + lane*16), so the
// XOR swizzle that makes the ds_read_b128 fragment loads conflict-free (chunk ^= (row>>1)&7) is applied to the
// per-lane SOURCE address; the fragment reads apply the same involution.  Two stages; the loads of K-step t+1
// are issued before the MFMAs of step t and drained by the barrier that ends the step.
//
// Operand orientation: for ordinary tiles the MFMA computes C^T fragments (first operand = W rows), so a lane owns
// 4 CONSECUTIVE output columns of one row: bias/residual/stores are 8/16-byte vector accesses and, with the W-row
// permutation 16*(a>>2)+4j+(a&3), a lane's 16 values are 16 consecutive columns.  Tiles that take the RoPE epilogue
// keep the identity column map (partner channel d+16 = next fragment, same lane/register); V tiles that are written
// in the packed VT layout use the un-swapped orientation (a lane owns 4 consecutive TOKENS of one channel).
//
// This file: the five kernels and their launchers.  gemm_glds_epilogue.h: what drains an accumulator block.  gemm_glds_tile.h: what
// the kernels share around their K-loops, and which pieces each kernel keeps as its own text because a shared form changes its code.
#include "gemm_glds_tile.h"

// BK_ = 64 (128-B LDS rows) or 32 (64-B rows: half the LDS per stage, so two 8-wave workgroups share a CU and one's
// prologue/epilogue runs under the other's K-loop); WGS_PER_CU is the co-residency the register budget is sized for.
// EPI selects the epilogue family compiled into an instantiation (the launcher picks the instantiation from the descriptor):
//   GLDS_EPI_BF16: bf16 stores without residual — plain / activation / RoPE tiles, VT tiles, folded LayerNorm (qkv, fc1, q / kv
//                  projections, convolutions);   GLDS_EPI_F32: fp32 output (+ fp32 residuals, bf16 twin, row statistics: proj,
//                  fc2, embeddings);   GLDS_EPI_BS: the same sub-layers on a bf16 residual stream (bf16 output + bf16 residuals +
//                  row statistics);   GLDS_EPI_ALL: the generic drain next to the fast families (everything else).
// One family per kernel keeps the register allocation of the 128-VGPR K-loop out of reach of epilogue code it never runs:
// with all of them inlined into one function, every option added to one epilogue spilled DMA pointers inside the K-loop.

// Launch geometry of an instantiation, stated once: the kernel lays its LDS image out by it and glds_launch_tile launches with it.
template <int BM_, int BN_, int WAVES_M, int WAVES_N, int STAGES, int BK_>
struct GldsTileGeom {
    static constexpr int THREADS = WAVES_M * WAVES_N * 64;
    static constexpr int STAGE_BYTES = (BM_ + BN_) * BK_ * 2;      // (BM + BN) LDS rows of BK 16-bit elements
    static constexpr int LDS_BYTES = STAGES * STAGE_BYTES;         // the ring; behind the K-loop the epilogues' bounce space
    static_assert(LDS_BYTES >= THREADS / 64 * GLDS_BOUNCE_BYTES, "bounce space");
};

// (This kernel keeps the text around its K-loop: with any one of glds_stagger / glds_kernarg_params in it, its 128x128 and 32-deep
//  instantiations compile to other code — profiles/gemm_glds_tile_codegen.txt.)
template <int BM_, int BN_, int WAVES_M, int WAVES_N, int STAGES, int A_MODE, int BK_ = 64, int WGS_PER_CU = 1, int EPI = GLDS_EPI_ALL, bool F16 = false>
__global__ __launch_bounds__(WAVES_M* WAVES_N * 64, WGS_PER_CU * WAVES_M * WAVES_N / 4) void gemm_bf16_glds_kernel(GldsParams p) {
    using GEOM = GldsTileGeom<BM_, BN_, WAVES_M, WAVES_N, STAGES, BK_>;
    static_assert(BN_ / WAVES_N == 64, "a wave owns 64 output columns (one 64-wide head)");
    constexpr int WTM = BM_ / WAVES_M;
    constexpr int FA = WTM / 16;          // A-row fragments per wave (4 or 8)
    static_assert(WTM % 16 == 0 && (FA == 4 || FA == 8), "wave tile rows");
    constexpr int NW = WAVES_M * WAVES_N;
    static_assert(BK_ == 64 || BK_ == 32, "K-step");
    constexpr int ROWB = BK_ * 2;         // bytes per LDS row
    constexpr int CPR = ROWB / 16;        // 16-byte chunks per row (8 or 4)
    constexpr int RPI = 1024 / ROWB;      // rows per 1-KiB DMA instruction (8 or 16)
    constexpr int STAGE_BYTES = GEOM::STAGE_BYTES;
    constexpr int NI = (BM_ + BN_) / RPI; // 1-KiB DMA instructions per stage
    constexpr int PER = NI / NW;          // per wave
    static_assert(NI % NW == 0, "DMA instructions must split evenly over the waves");

    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned long long tr0 = 0, tr1 = 0, tr2 = 0;
    if (UC_TRACE(p)) tr0 = __builtin_amdgcn_s_memrealtime();
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave / WAVES_N, wc = wave % WAVES_N;
    const int nwg = p.tiles_m * p.tiles_n;
    constexpr bool FUSE2_OK = BM_ == 128 && BN_ == 128;   // fused two-way K split (fuse_split2): this tile only (dense and conv, bf16 and fp16)
    const bool fuse2 = FUSE2_OK && p.fuse_split2;
    const int ksplit = fuse2 ? ((int)blockIdx.x >= nwg ? 1 : 0)
                             : (p.split_k > 1 ? (int)uc_div(blockIdx.x, p.dNwg) : 0);   // split-K slice
    const int t = xcd_remap((int)blockIdx.x - ksplit * nwg, nwg);
    // Tile order inside an XCD's run: groups of GM row panels swept column by column, so the ~32 tiles an XCD runs
    // concurrently form a GM x (32/GM) block that shares GM A-panels and 32/GM W-panels in its L2 (a plain row-major
    // order shares 2 A-panels but streams ALL of W through every pair of row panels: 2.4x algorithmic fetch traffic).
    int tm, tn;
    {
        const int GM = p.group_m;
        const int per_group = GM * p.tiles_n;
        const int grp = (int)uc_div((unsigned)t, p.dPerGroup), within = t - grp * per_group;
        const int first_m = grp * GM;
        const bool last = p.tiles_m - first_m < GM;                        // the ragged last group has tiles_m % GM row panels
        const int gsz = last ? p.tiles_m - first_m : GM;
        tn = (int)uc_div((unsigned)within, last ? p.dGmLast : p.dGm);
        tm = first_m + within - tn * gsz;
    }
    if (p.stagger > 0 && blockIdx.x < 256u * WGS_PER_CU) {
        // Experiment (UC_GEMM_STAGGER, off by default): de-phase the CUs.  Every tile of a launch costs the same, so all 256 CUs
        // reach their epilogues together and the store / residual traffic hits HBM as one burst while the matrix pipes idle.
        // The first round of workgroups (one per CU) starts in 8 phase groups chosen by ROW PANEL, so the column tiles that
        // share an A panel through their XCD's L2 stay in step; the offsets persist down each CU's chain of tiles.
        const unsigned phase = (unsigned)tm & 7u;
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
        const unsigned long long wait = (unsigned long long)phase * (unsigned)p.stagger;
        while (__builtin_amdgcn_s_memrealtime() - t0 < wait) __builtin_amdgcn_s_sleep(16);
    }
    const int64_t m0 = (int64_t)tm * BM_;
    const int64_t n0 = (int64_t)tn * BN_;
    const int64_t wave_m = m0 + wr * WTM;
    const int64_t wave_n = n0 + wc * 64;

    // ---- per-wave epilogue mode (wave-uniform) ----
    const bool is_vt = A_MODE == UC_A_DENSE && p.vt_col0 >= 0 && wave_n >= p.vt_col0;        // conv tiles take neither epilogue
    const bool is_rope = A_MODE == UC_A_DENSE && !is_vt && p.rope_cols > 0 && wave_n < p.rope_cols;
    const int mode = is_vt ? 2 : (is_rope ? 1 : 0);

    // ---- DMA sources: instruction I = wave*PER + q covers combined-tile rows [RPI*I, RPI*(I+1)) ----
    // Dense: one 64-bit source pointer per instruction, advanced by k0.
    // Conv: buffer-addressed DMA.  Two wave-uniform descriptors (the input window of this tile, shifted back by one image
    // row + one pixel so that tap (ky,kx) is a non-negative uniform soffset, and the tile's weight rows); per instruction a
    // 32-bit byte offset of the lane's row and a 9-bit mask of the taps that fall inside the image.  A tap in the zero
    // padding sets the lane's offset to 0xffffffff: out of the descriptor's range, and the hardware writes zeros to LDS
    // (tools/probes/buffer_lds.hip) — no 64-bit per-lane address math, no padding source, half the address registers.
    const bf16_t* src[A_MODE == UC_A_DENSE ? PER : 1];
    unsigned st0[A_MODE == UC_A_DENSE ? 1 : PER], st1[A_MODE == UC_A_DENSE ? 1 : PER];
    uint4_t srd_a = (uint4_t){0u, 0u, 0u, 0u}, srd_w = srd_a;
    if constexpr (A_MODE != UC_A_DENSE) {
        const int b0 = (int)uc_div((unsigned)min(m0, p.M - 1), p.dHWo);     // < 2^30 output pixels (launcher-checked)
        srd_a = make_srd(p.A + ((int64_t)b0 * p.cH * p.cW - (p.cW + 1)) * p.cCin);
        srd_w = make_srd(p.W + min(n0, p.N - 1) * p.K);
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const int rr = (wave * PER + q) * RPI + lane / CPR;
            const int c = (lane % CPR) ^ glds_swz<BK_>(rr);
            if (rr < BM_) {
                const unsigned m = (unsigned)min(m0 + rr, p.M - 1);          // < 2^30 output pixels (launcher-checked)
                const unsigned mrow = uc_div(m, p.dWo);
                const int ox = (int)(m - mrow * (unsigned)p.cWo) * p.cStride;
                const unsigned b = uc_div(mrow, p.dHo);
                const int oy = (int)(mrow - b * (unsigned)p.cHo) * p.cStride;
                st0[q] = (unsigned)((((int64_t)((int)b - b0) * p.cH + oy) * p.cW + ox) * p.cCin + c * 8) * 2u;
                unsigned colmask = 0, mask = 0;
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) colmask |= ((unsigned)(ox - 1 + kx) < (unsigned)p.cW ? 1u : 0u) << kx;
#pragma unroll
                for (int ky = 0; ky < 3; ++ky) mask |= ((unsigned)(oy - 1 + ky) < (unsigned)p.cH ? colmask : 0u) << (3 * ky);
                st1[q] = mask;
            } else {
                const int64_t n = min(n0 + (rr - BM_), p.N - 1);
                st0[q] = (unsigned)((n - min(n0, p.N - 1)) * p.K + c * 8) * 2u;
                st1[q] = 0x1ffu;
            }
        }
    } else {
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const int rr = (wave * PER + q) * RPI + lane / CPR;
            const int c = (lane % CPR) ^ glds_swz<BK_>(rr);   // logical chunk stored at physical chunk (lane % CPR) of row rr
            if (rr < BM_) src[q] = p.A + min(m0 + rr, p.M - 1) * p.lda + c * 8;
            else src[q] = p.W + min(n0 + (rr - BM_), p.N - 1) * p.K + c * 8;
        }
    }
    const unsigned lds_base = lds_addr(smem);   // LDS byte address of the dynamic region
    auto issue_stage = [&](int stage, int64_t k0) {
        int tap = 0;
        unsigned soff_a = 0, soff_w = 0;
        if constexpr (A_MODE != UC_A_DENSE) {
            tap = (int)uc_div((unsigned)k0, p.dCin);
            const int ch0 = (int)k0 - tap * p.cCin;
            const int ky = tap / 3, kx = tap - 3 * ky;
            soff_a = (unsigned)(((ky * p.cW + kx) * p.cCin + ch0) * 2);
            soff_w = (unsigned)(k0 * 2);
        }
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const unsigned dst = __builtin_amdgcn_readfirstlane(lds_base + (unsigned)(stage * STAGE_BYTES + wave * (PER * 1024) + q * 1024));
            if constexpr (A_MODE == UC_A_DENSE) {
                dma16_to_lds(src[q] + k0, dst);
            } else {
                const bool is_a = (wave * PER + q) * RPI < BM_;   // wave-uniform: an instruction is all-A or all-W
                const unsigned vo = ((st1[q] >> tap) & 1u) ? st0[q] : 0xffffffffu;
                if (is_a && UC_DBG(p, 64) && tap != 0) continue;   // diagnostics (wrong results): A tiles staged for tap 0 only — what a halo-tiled form could save at most
                if (is_a) dma16_buf_to_lds(vo, srd_a, soff_a, dst);
                else dma16_buf_to_lds(vo, srd_w, soff_w, dst);
            }
        }
    };

    // ---- fragment addressing (identity row maps: conflict-free under the (row>>1)&7 chunk swizzle) ----
    // Row r of fragment i is wr*WTM + 16 i + frow (A) / BM + wc*64 + 16 j + frow (W): the swizzle key (r>>1)&7 only depends
    // on frow (all other terms are multiples of 16), and the row offsets are one base + compile-time multiples of 2 KiB —
    // two base registers and two swizzled chunk offsets (one per 32-wide K half) address all 8..12 fragment reads.
    const int frow = lane & 15;
    const int fk = lane >> 4;
    const int f_sw = glds_swz<BK_>(frow);
    const int a_base = (wr * WTM + frow) * ROWB;
    const int w_base = (BM_ + wc * 64 + frow) * ROWB;
    const int ch_off[2] = {((0 * 4 + fk) ^ f_sw) << 4, ((1 * 4 + fk) ^ f_sw) << 4};   // [1] unused when BK_ == 32

    float4_t acc[FA][4];
#pragma unroll
    for (int i = 0; i < FA; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (float4_t){0.f, 0.f, 0.f, 0.f};

    // K range of this workgroup (whole K unless split_k > 1)
    const int nk_total = (int)(p.K / BK_);
    const int nsplit = fuse2 ? 2 : p.split_k;
    const int nk_per = (nk_total + nsplit - 1) / nsplit;
    const int kt0 = ksplit * nk_per;
    int nk = max(0, min(nk_per, nk_total - kt0));
    if UC_DBG(p, 8) nk = min(nk, 1);                      // diagnostics: one K-step only (launch + prologue + epilogue cost)
    const int64_t kbase = (int64_t)kt0 * BK_;
    // SWAP: first MFMA operand = W rows -> C^T fragments (lane owns 4 consecutive columns of one row);
    // !SWAP (VT tiles): first operand = A rows (lane owns 4 consecutive tokens of one channel).
    auto compute_stage = [&](const char* st, auto swap_tag, auto&& mid) {
        constexpr bool SWAP = decltype(swap_tag)::value;
#pragma unroll
        for (int ks = 0; ks < BK_ / 32; ++ks) {
            bf16x8_t af[FA];
#pragma unroll
            for (int i = 0; i < FA; ++i) {
                uint4 raw = *reinterpret_cast<const uint4*>(st + a_base + ch_off[ks] + i * 16 * ROWB);
                if constexpr (A_MODE != UC_A_DENSE) {
                    if (p.relu_a) raw = relu_bf16x8(raw);   // uniform flag: ReLU of the DPT residual conv unit, applied on load
                }
                af[i] = __builtin_bit_cast(bf16x8_t, raw);
            }
            if constexpr (A_MODE == UC_A_DENSE) {
                bf16x8_t wf[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) wf[j] = *reinterpret_cast<const bf16x8_t*>(st + w_base + ch_off[ks] + j * 16 * ROWB);
#pragma unroll
                for (int i = 0; i < FA; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if constexpr (SWAP) acc[i][j] = glds_mfma<F16>(wf[j], af[i], acc[i][j]);
                        else acc[i][j] = glds_mfma<F16>(af[i], wf[j], acc[i][j]);
                    }
            } else {
                // conv tiles carry more loop state (offsets, tap masks, two descriptors): W fragments are read one at a time
                // (20 instead of 32 fragment registers) so that nothing spills inside the K-loop
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bf16x8_t wf = *reinterpret_cast<const bf16x8_t*>(st + w_base + ch_off[ks] + j * 16 * ROWB);
#pragma unroll
                    for (int i = 0; i < FA; ++i) acc[i][j] = glds_mfma<F16>(wf, af[i], acc[i][j]);
                }
            }
            if (ks == 0) mid();
        }
    };
    auto main_loop = [&](auto swap_tag) {
        if constexpr (STAGES == 2) {
            // 2-stage ring: the DMA of step kt+1 is in flight while the MFMAs of step kt run.
            if (nk > 0) issue_stage(0, kbase);
            for (int kt = 0; kt < nk; ++kt) {
                wait_vmcnt<0>();                 // this wave's pieces of stage kt have landed
                if (!UC_DBG(p, 2)) __builtin_amdgcn_s_barrier();    // ... and everyone else's; every wave is done reading stage kt-1
                if (UC_TRACE(p) && kt == 0) tr1 = __builtin_amdgcn_s_memrealtime();
                asm volatile("" ::: "memory");
                // where the next stage's DMA is issued (same-box A/B): dense pieces cost one 64-bit add each and go first
                // (behind the first MFMA group they lost 0-5 %, split between the wave halves of a SIMD 2-8 %); conv pieces
                // carry the tap test, s_nop 4 and a descriptor select and go behind the wave's first 16 queued MFMAs (+5 % on
                // the 256-channel convs)
                if constexpr (A_MODE == UC_A_DENSE) {
                    if (kt + 1 < nk && !UC_DBG(p, 1)) issue_stage((kt + 1) & 1, kbase + (int64_t)(kt + 1) * BK_);
                    compute_stage(smem + (kt & 1) * STAGE_BYTES, swap_tag, [] {});
                } else {
                    compute_stage(smem + (kt & 1) * STAGE_BYTES, swap_tag, [&] {
                        if (kt + 1 < nk && !UC_DBG(p, 1)) issue_stage((kt + 1) & 1, kbase + (int64_t)(kt + 1) * BK_);
                    });
                }
            }
        } else {
            // 3-stage ring, DMA two K-steps ahead: the loads of step kt+1 stay in flight across the barrier of step kt.
            // (A 4-stage ring of the 128x128 tile — three steps ahead — was measured at 1 pair per batch, where every K-step is a wait
            // for its own DMA: 8.49 vs 8.57 ms per forward, within noise; not kept.)
            if (nk > 0) issue_stage(0, kbase);
            if (nk > 1) issue_stage(1, kbase + BK_);
            int cur = 0;
            for (int kt = 0; kt < nk; ++kt) {
                if (kt + 1 < nk) wait_vmcnt<PER>(); else wait_vmcnt<0>();
                __builtin_amdgcn_s_barrier();
                if (UC_TRACE(p) && kt == 0) tr1 = __builtin_amdgcn_s_memrealtime();
                asm volatile("" ::: "memory");
                int nxt = cur + 2; if (nxt >= 3) nxt -= 3;
                if (kt + 2 < nk) issue_stage(nxt, kbase + (int64_t)(kt + 2) * BK_);
                compute_stage(smem + cur * STAGE_BYTES, swap_tag, [] {});
                cur = (cur == 2) ? 0 : cur + 1;
            }
        }
    };
    if constexpr (A_MODE == UC_A_DENSE) {
        if (mode == 2) main_loop(std::false_type{}); else main_loop(std::true_type{});
    } else {
        main_loop(std::true_type{});
    }

    if constexpr (FUSE2_OK) {
        if (fuse2) {
            // Fused two-way K split.  The producers are the LOW block ids: the dispatcher starts them first and they never wait, so a
            // consumer that spins always has a partner that is running or has finished — also when two such launches share the CUs
            // (the decoder's two view streams).  The hand-over buffer is UNCACHED device memory (hipDeviceMallocUncached: no L2 on
            // either side, so partners on different XCDs — whose L2s are not coherent — need no buffer_wbl2 / buffer_inv, which
            // write back / invalidate a whole L2 and cost more than the split saves: measured); the flag is polled with volatile
            // (L1-bypassing) loads; ordering by s_waitcnt + barrier.
            float* ws = p.fs_ws + (size_t)t * (128 * 128) + (size_t)tid * 4;
            volatile unsigned* flag = p.fs_flags + t;
            if (ksplit == 0) {
#pragma unroll
                for (int i = 0; i < FA; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) *reinterpret_cast<float4_t*>(ws + (size_t)(i * 4 + j) * (NW * 64 * 4)) = acc[i][j];
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this thread's partial sums are in memory
                __syncthreads();                                        // ... everyone's
                if (tid == 0) *flag = 1u;
                return;
            }
            if (tid == 0) {
                while (*flag != 1u) __builtin_amdgcn_s_sleep(4);
            }
            __syncthreads();
            asm volatile("" ::: "memory");
            {   // (plain loads, all 16 in flight: the buffer is uncached memory, and no line of it can sit in this CU's L1 — a volatile
                //  access would be waited for one by one, 16 round trips)
                float4_t part[FA][4];
#pragma unroll
                for (int i = 0; i < FA; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) part[i][j] = *reinterpret_cast<const float4_t*>(ws + (size_t)(i * 4 + j) * (NW * 64 * 4));
#pragma unroll
                for (int i = 0; i < FA; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] += part[i][j];
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (tid == 0) *flag = 0u;            // for the next launch on this stream / the next graph replay
        }
    }

    // The epilogue's parameters are re-read from the kernarg segment HERE.  Carried through the K-loop in SGPRs (some 60 of
    // them: pointers, leading dimensions, option words) they overflowed the scalar file, the overflow went to VGPR lanes, and
    // the 128-VGPR K-loop answered with scratch reloads of its DMA source pointers inside the loop.
#if defined(__HIP_DEVICE_COMPILE__)
    const __attribute__((opencl_constant)) GldsParams* kp =
        (const __attribute__((opencl_constant)) GldsParams*)__builtin_amdgcn_kernarg_segment_ptr();   // explicit arguments start at offset 0
    asm volatile("" : "+s"(kp)::"memory");
    glds_pe_t pe = *kp;
#else
    glds_pe_t pe = p;
#endif
    if UC_DBG(pe, 4) {                                     // diagnostics: no epilogue (keeps the accumulators live)
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < FA; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) s += acc[i][j][0] + acc[i][j][1] + acc[i][j][2] + acc[i][j][3];
        if (s == 12345.678f) reinterpret_cast<float*>(pe.C)[0] = s;
        return;
    }
    // every wave is done with the last stage: the ring becomes the epilogue's bounce space (GldsTileGeom asserts that it holds it)
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (UC_TRACE(pe)) tr2 = __builtin_amdgcn_s_memrealtime();
    glds_epilogue_dispatch<FA, A_MODE, EPI, F16>(pe, acc, mode, wave_m, wave_n, tid, wave, ksplit, smem);
    if (UC_TRACE(pe)) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (tid == 0) {
            unsigned hw;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
            unsigned xcc;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
            unsigned long long* t = UC_TRACE(pe) + (size_t)blockIdx.x * 6;
            t[0] = tr0; t[1] = tr1; t[2] = tr2; t[3] = __builtin_amdgcn_s_memrealtime(); t[4] = hw; t[5] = xcc;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Eight-wave form of the dense 256x256x64 tile: 2 x 4 waves of 128x64 (two waves per SIMD, 256 registers each).
//
// The 16-wave kernel above has 128 registers per wave: accumulators (64) + one K-half of fragments (32) fill them, so every
// fragment is read from LDS right before its MFMAs — after each barrier the matrix pipes wait for the first ds_reads of all
// 16 waves, and a 64x64 wave tile moves 512 B of LDS per MFMA.  Here a wave owns 128x64: 12 fragment reads feed 32 MFMAs
// (384 B per MFMA), and the registers hold the NEXT 32-deep K-chunk's fragments while the current chunk's MFMAs run:
//
//   chunk 0 of stage s:  MFMAs on (a, w)   | ds_read chunk 1 of stage s   -> (a, wn)       (a is refilled row block by row block)
//   mid-step:            s_waitcnt + s_barrier: everyone has READ stage s, everyone's DMA of stage s+1 has landed
//                        DMA of stage s+2 -> buffer of stage s
//   chunk 1 of stage s:  MFMAs on (a, wn)  | ds_read chunk 0 of stage s+1 -> (a, w)
//
// One barrier per K-step as before, but every wave arrives at it with 32 MFMAs' worth of operands already in registers.
template <int EPI>
struct Glds8Geom {      // LDS image: two stages of (256 + 256) rows x 128 B | side panel (BF16 family)
    static constexpr int THREADS = 512, STAGE_BYTES = (256 + 256) * 128;
    static constexpr int LDS_BYTES = 2 * STAGE_BYTES + (EPI == GLDS_EPI_BF16 ? GLDS_SIDE_BYTES : 0);
    static_assert(2 * STAGE_BYTES >= THREADS / 64 * GLDS_BOUNCE_BYTES, "bounce space");
};

template <int EPI>
__global__ __launch_bounds__(Glds8Geom<EPI>::THREADS, 2) void gemm_bf16_glds8_kernel(GldsParams p) {
    constexpr int BM_ = 256, BN_ = 256, WAVES_N = 4, FA = 8, ROWB = 128, STAGE_BYTES = Glds8Geom<EPI>::STAGE_BYTES, PER = 8, RPI = 8, CPR = 8;
    constexpr int A_MODE = UC_A_DENSE;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned long long tr0 = 0, tr1 = 0, tr2 = 0;
    if (UC_TRACE(p)) tr0 = __builtin_amdgcn_s_memrealtime();
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave / WAVES_N, wc = wave % WAVES_N;
    const int nwg = p.tiles_m * p.tiles_n;
    const int ksplit = p.split_k > 1 ? (int)uc_div(blockIdx.x, p.dNwg) : 0;
    const int t = xcd_remap((int)blockIdx.x - ksplit * nwg, nwg);
    int tm, tn;
    {   // tile order: see the 16-wave kernel
        const int GM = p.group_m;
        const int per_group = GM * p.tiles_n;
        const int grp = (int)uc_div((unsigned)t, p.dPerGroup), within = t - grp * per_group;
        const int first_m = grp * GM;
        const bool last = p.tiles_m - first_m < GM;
        const int gsz = last ? p.tiles_m - first_m : GM;
        tn = (int)uc_div((unsigned)within, last ? p.dGmLast : p.dGm);
        tm = first_m + within - tn * gsz;
    }
    glds_stagger(p, tm, 256u);
    const int64_t m0 = (int64_t)tm * BM_;
    const int64_t n0 = (int64_t)tn * BN_;
    const int64_t wave_m = m0 + wr * 128;
    const int64_t wave_n = n0 + wc * 64;
    const bool is_vt = p.vt_col0 >= 0 && wave_n >= p.vt_col0;
    const bool is_rope = !is_vt && p.rope_cols > 0 && wave_n < p.rope_cols;
    const int mode = is_vt ? 2 : (is_rope ? 1 : 0);

    // DMA sources.  Instruction I = wave*8 + q covers combined-tile rows [8 I, 8 I + 8): waves 0-3 stage the A rows, waves 4-7 the
    // W rows, 64 rows each.  The 8-row groups of a wave are one uniform stride apart, so a piece is addressed as a wave-uniform
    // 64-bit base (SGPR pair, advanced on the scalar unit) + one of TWO per-lane byte offsets (the chunk swizzle key
    // (row >> 1) & 7 only depends on the parity of q) — 2 address registers instead of 16.  Row groups past the matrix end are
    // clamped to its last 8 rows as a group (launcher: M % 8 == 0, N % 8 == 0); their products are never stored.
    const bool stages_a = wave < 4;
    const int64_t ld_src = stages_a ? p.lda : p.K;
    const bf16_t* sbase[PER];
    {
        const bf16_t* mat = stages_a ? p.A : p.W;
        const int64_t row0 = (stages_a ? m0 : n0) + (wave & 3) * 64, lim = (stages_a ? p.M : p.N) - 8;
#pragma unroll
        for (int q = 0; q < PER; ++q) sbase[q] = mat + min(row0 + 8 * q, lim) * ld_src;
    }
    const unsigned voff_row = (unsigned)((lane >> 3) * (int)ld_src) * 2u;
    const unsigned voff2[2] = {voff_row + (unsigned)(((lane & 7) ^ (lane >> 4)) << 4), voff_row + (unsigned)(((lane & 7) ^ (4 + (lane >> 4))) << 4)};
    const unsigned lds_base = lds_addr(smem);
    auto issue_piece = [&](int stage, int64_t k0, int q) __attribute__((always_inline)) {
        const unsigned dst = __builtin_amdgcn_readfirstlane(lds_base + (unsigned)(stage * STAGE_BYTES + wave * (PER * 1024) + q * 1024));
        dma16_s_to_lds(voff2[q & 1], sbase[q] + k0, dst);
    };
    auto issue_stage = [&](int stage, int64_t k0) __attribute__((always_inline)) {
#pragma unroll
        for (int q = 0; q < PER; ++q) issue_piece(stage, k0, q);
    };
    // side panel (see GLDS_SIDE_*): one 1-KiB piece per wave, issued BEFORE the first stage's pieces — loads return in order, so the
    // first K-step's vmcnt(0) + barrier cover it.  Out-of-range rows / columns are clamped (their products are never stored).
    const bool side_on = EPI == GLDS_EPI_BF16 && p.side_lds != 0;
    if (EPI == GLDS_EPI_BF16 && side_on) {
        const unsigned dst = __builtin_amdgcn_readfirstlane(lds_base + (unsigned)(2 * STAGE_BYTES + wave * 1024));
        if (wave < 2) {             // (mean, rstd) of rows 128 wave + 2 lane, + 1
            const int r = (int)min((int64_t)(128 * wave + 2 * lane), p.M - 2 - m0);
            dma16_s_to_lds((unsigned)r * 8u, p.ln_stats + m0, dst);
        } else if (wave == 2) {     // column sums of columns 4 lane .. + 3
            const int c = (int)min((int64_t)(4 * lane), p.N - 4 - n0);
            dma16_s_to_lds((unsigned)c * 4u, p.ln_colsum + n0, dst);
        } else if (wave == 3) {     // bias
            const int c = (int)min((int64_t)(4 * lane), p.N - 4 - n0);
            dma16_s_to_lds((unsigned)c * 4u, p.bias + n0, dst);
        } else if (p.rope_cols > 0) {   // (y, x) of row 64 (wave - 4) + lane
            const int r = (int)min((int64_t)(64 * (wave - 4) + lane), p.M - 1 - m0);
            dma16_s_to_lds((unsigned)r * 16u, p.rope_pos + m0 * 2, dst);
        }
    }

    const int frow = lane & 15;
    const int fk = lane >> 4;
    const int f_sw = glds_swz<64>(frow);
    const int a_base = (wr * 128 + frow) * ROWB;
    const int w_base = (BM_ + wc * 64 + frow) * ROWB;
    const int ch_off[2] = {((0 * 4 + fk) ^ f_sw) << 4, ((1 * 4 + fk) ^ f_sw) << 4};

    float4_t acc[FA][4];
#pragma unroll
    for (int i = 0; i < FA; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (float4_t){0.f, 0.f, 0.f, 0.f};

    const int nk_total = (int)(p.K / 64);
    const int nk_per = (nk_total + p.split_k - 1) / p.split_k;
    const int kt0 = ksplit * nk_per;
    int nk = max(0, min(nk_per, nk_total - kt0));
    if UC_DBG(p, 8) nk = min(nk, 1);
    const int64_t kbase = (int64_t)kt0 * 64;

    auto main_loop = [&](auto swap_tag) __attribute__((always_inline)) {
        constexpr bool SWAP = decltype(swap_tag)::value;
        if (nk <= 0) return;
        bf16x8_t a[FA], w[4], wn[4];
        auto rd_a = [&](const char* st, int ks, int i) __attribute__((always_inline)) {
            return *reinterpret_cast<const bf16x8_t*>(st + a_base + ch_off[ks] + i * 16 * ROWB);
        };
        auto rd_w = [&](const char* st, int ks, int j) __attribute__((always_inline)) {
            return *reinterpret_cast<const bf16x8_t*>(st + w_base + ch_off[ks] + j * 16 * ROWB);
        };
        auto mma = [&](int i, int j, bf16x8_t av, bf16x8_t wv) __attribute__((always_inline)) {
            if constexpr (SWAP) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wv, av, acc[i][j], 0, 0, 0);
            else acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, wv, acc[i][j], 0, 0, 0);
        };
        issue_stage(0, kbase);
        wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();
        if (UC_TRACE(p)) tr1 = __builtin_amdgcn_s_memrealtime();
        asm volatile("" ::: "memory");
        if (nk > 1) issue_stage(1, kbase + 64);
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = rd_w(smem, 0, j);
#pragma unroll
        for (int i = 0; i < FA; ++i) a[i] = rd_a(smem, 0, i);
        // chunk 0 of a stage: MFMAs on (a, w) while chunk 1 of the same stage streams into (a, wn).  The scheduling fences keep
        // every refill of a[i] behind the MFMAs that read the old a[i]: hoisted, both generations are live and the loop spills.
        auto chunk0 = [&](const char* cur) __attribute__((always_inline)) {
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < FA; ++i) {
#pragma unroll
                for (int j = 0; j < 4; ++j) mma(i, j, a[i], w[j]);
                __builtin_amdgcn_sched_barrier(0);
                if (i == 0) {      // behind the first MFMA group: in front of it the group would wait for these four reads as well
#pragma unroll
                    for (int j = 0; j < 4; ++j) wn[j] = rd_w(cur, 1, j);
                }
                a[i] = rd_a(cur, 1, i);
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        // One K-step but the last: chunk 0, the mid-step synchronisation, chunk 1 with the next stage's first fragments streaming
        // in.  DMA (compile-time): the DMA of stage kt + 2 goes into the buffer just released, one 1-KiB piece behind each MFMA
        // group (issued as a block in front of chunk 1 its ~80 scalar instructions hold back both waves of a SIMD right after
        // the barrier).  The loop bodies are straight-line: with the last steps' DMA-free / prefetch-free forms inside one loop
        // the accumulators went through phi copies (90 of them parked in scratch) and every join cost an lgkmcnt(0).
        // (the loops are rotated so that their headers sit at the synchronisation point: hipcc drains lgkmcnt at a loop header
        // whatever is pending, and there the drain is wanted)
        auto step = [&](int kt, auto dma_tag) __attribute__((always_inline)) {
            constexpr bool DMA = decltype(dma_tag)::value;
            const char* nxt = smem + ((kt + 1) & 1) * STAGE_BYTES;
            // every fragment of stage kt is in registers (lgkmcnt(0)), this wave's DMA pieces of the next stage have landed
            // (vmcnt(0)); after the barrier both hold for the whole workgroup
            if UC_DBG(p, 32) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // diagnostics: do not wait for the DMA (wrong results)
            else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            const int64_t k2 = kbase + (int64_t)(kt + 2) * 64;
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < 4; ++j) w[j] = rd_w(nxt, 0, j);
#pragma unroll
            for (int i = 0; i < FA; ++i) {
#pragma unroll
                for (int j = 0; j < 4; ++j) mma(i, j, a[i], wn[j]);
                __builtin_amdgcn_sched_barrier(0);
                a[i] = rd_a(nxt, 0, i);
                if constexpr (DMA) { if (!UC_DBG(p, 1)) issue_piece(kt & 1, k2, i); }
                __builtin_amdgcn_sched_barrier(0);
            }
            chunk0(nxt);
        };
        chunk0(smem);
        for (int kt = 0; kt + 2 < nk; ++kt) step(kt, std::true_type{});
        if (nk > 1) step(nk - 2, std::false_type{});
#pragma unroll
        for (int i = 0; i < FA; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) mma(i, j, a[i], wn[j]);
    };
    if (mode == 2) main_loop(std::false_type{}); else main_loop(std::true_type{});

    glds_pe_t pe = *glds_kernarg_params(p);
    if UC_DBG(pe, 4) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < FA; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) s += acc[i][j][0] + acc[i][j][1] + acc[i][j][2] + acc[i][j][3];
        if (s == 12345.678f) reinterpret_cast<float*>(pe.C)[0] = s;
        return;
    }
    __builtin_amdgcn_s_barrier();          // every wave is done with the ring: it becomes the bounce space (8 KiB per wave)
    asm volatile("" ::: "memory");
    if (UC_TRACE(pe)) tr2 = __builtin_amdgcn_s_memrealtime();
    glds_epilogue_dispatch<FA, A_MODE, EPI>(pe, acc, mode, wave_m, wave_n, tid, wave, ksplit, smem,
                                            (EPI == GLDS_EPI_BF16 && pe.side_lds) ? smem + 2 * STAGE_BYTES : nullptr);
    if (UC_TRACE(pe)) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (tid == 0) {
            unsigned hw;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
            unsigned xcc;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
            unsigned long long* t = UC_TRACE(pe) + (size_t)blockIdx.x * 6;
            t[0] = tr0; t[1] = tr1; t[2] = tr2; t[3] = __builtin_amdgcn_s_memrealtime(); t[4] = hw; t[5] = xcc;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Four-wave form of the dense 256x256x64 tile: 2 x 2 waves of 128x128, ONE wave per SIMD, 256 accumulators per lane pinned in
// a0..a255 and a hand-scheduled K-loop (gemm_glds4_loop.inc, generated by gen/gen_glds4_loop.py) — the layout of the vendor's
// hand-written kernels: 32 ds_read_b128 feed 128 MFMAs per wave per K-step (256 B of LDS per MFMA against 512 B for the 64x64 wave
// tiles of the 16-wave kernel), so the same FLOPs cost less LDS traffic — less energy, on a part that runs this kernel at its power
// cap.  hipcc cannot schedule this form (accumulator copies and scratch in the loop), hence the inline-asm loop; the
// prologue (tile order, DMA source set-up) and the epilogues are the shared C++ ones: after the loop each wave drains its 128x128
// tile as two 128x64 halves through glds_epilogue_dispatch<8, ...>.
//
// Measured (round 3).  First schedule (all 16 pieces behind ONE mid-step barrier with vmcnt(0)): on par with the
// 16-wave kernel (8192^3: 1384-1400 vs 1343-1412 TFLOP/s) — a piece had 1000-2000 cycles to land, less than the loaded latency.  Second
// schedule (two barriers per step, counted vmcnt(16), a piece behind every fifth MFMA: gen/gen_glds4_loop.py `step`): 8192^3 1535
// (the vendor's hand-written kernel of the same design: 1543), K = 4096 shapes +5.6 % over the 16-wave kernel, K = 1024 shapes +-1 %
// (bound by the ~5.6 us a tile costs outside its K-loop).  Routed for K >= 2048 (UC_GEMM_4WAVE, UC_GEMM_4WAVE_MIN_K); gemm_variant 7.
//
// LDS image, stage ring, chunk swizzle and DMA piece addressing are those of the eight-wave kernel; waves 0-1 stage the A rows, waves
// 2-3 the W rows (128 rows = 16 pieces of 1 KiB each per stage).  The accumulators cross from the asm statement to the epilogue in
// the physical registers a0..a255 (read out by the v_accvgpr_read statements of UC_GLDS4_READ_HALF*): nothing between the loop and
// the last read-out may allocate an AGPR — tools/check_glds4_agprs.py verifies that on the compiled code (build.py runs it).
#include "gemm_glds4_loop.inc"

struct Glds4Geom {      // LDS image: two stages of (256 + 256) rows x 128 B
    static constexpr int THREADS = 256, STAGE_BYTES = (256 + 256) * 128, LDS_BYTES = 2 * STAGE_BYTES;
    static_assert(LDS_BYTES >= THREADS / 64 * GLDS_BOUNCE_BYTES, "bounce space");
};

template <int EPI>
__global__ __launch_bounds__(Glds4Geom::THREADS, 1) void gemm_bf16_glds4_kernel(GldsParams p) {
    constexpr int BM_ = 256, BN_ = 256, ROWB = 128, A_MODE = UC_A_DENSE;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int nwg = p.tiles_m * p.tiles_n;
    const int t = xcd_remap((int)blockIdx.x, nwg);
    int tm, tn;
    {   // tile order: see the 16-wave kernel
        const int GM = p.group_m;
        const int per_group = GM * p.tiles_n;
        const int grp = (int)uc_div((unsigned)t, p.dPerGroup), within = t - grp * per_group;
        const int first_m = grp * GM;
        const bool last = p.tiles_m - first_m < GM;
        const int gsz = last ? p.tiles_m - first_m : GM;
        tn = (int)uc_div((unsigned)within, last ? p.dGmLast : p.dGm);
        tm = first_m + within - tn * gsz;
    }
    glds_stagger(p, tm, 256u);
    const int64_t m0 = (int64_t)tm * BM_;
    const int64_t n0 = (int64_t)tn * BN_;
    const int64_t wave_m = m0 + wr * 128;
    const int64_t wave_n = n0 + wc * 128;
    // (launcher: rope_cols and vt_col0 are multiples of 128, so a wave's two 64-column halves share a mode)
    const bool is_vt = p.vt_col0 >= 0 && wave_n >= p.vt_col0;
    const bool is_rope = !is_vt && p.rope_cols > 0 && wave_n < p.rope_cols;
    const int mode = is_vt ? 2 : (is_rope ? 1 : 0);

    // DMA slab of this wave: 128 rows of A (waves 0, 1) or of W (waves 2, 3), 16 pieces of 8 rows
    const bool stages_a = wave < 2;
    const bf16_t* mat = stages_a ? p.A : p.W;
    const unsigned pitch = (unsigned)((stages_a ? p.lda : p.K) * 2);                       // bytes (launcher: < 2^31)
    const unsigned row0 = (unsigned)((stages_a ? m0 : n0) + (wave & 1) * 128);
    const unsigned lim = (unsigned)((stages_a ? p.M : p.N) - 8);
    const unsigned long long mat_u = (unsigned long long)mat;
    const unsigned base_lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)mat_u);
    const unsigned base_hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(mat_u >> 32));
    const unsigned voff_row = (unsigned)(lane >> 3) * pitch;
    const unsigned voff0 = voff_row + (unsigned)(((lane & 7) ^ (lane >> 4)) << 4);
    const unsigned voff1 = voff_row + (unsigned)(((lane & 7) ^ (4 + (lane >> 4))) << 4);
    const unsigned lds_base = lds_addr(smem);
    const unsigned lds_dma = (unsigned)__builtin_amdgcn_readfirstlane((int)(lds_base + (unsigned)wave * 16384u));
    // fragment read addresses of stage 0 (K halves 0 / 1): row frow of the wave's block 0, chunk (4 ks + fk) ^ swizzle(frow)
    const int frow = lane & 15, fk = lane >> 4, f_sw = glds_swz<64>(frow);
    const unsigned ch0 = (unsigned)(((0 * 4 + fk) ^ f_sw) << 4), ch1 = (unsigned)(((1 * 4 + fk) ^ f_sw) << 4);
    const unsigned a_row = lds_base + (unsigned)((wr * 128 + frow) * ROWB), w_row = lds_base + (unsigned)((BM_ + wc * 128 + frow) * ROWB);
    const unsigned nk = (unsigned)(p.K / 64);
    if (mode == 2) {
        asm volatile(UC_GLDS4_LOOP_NOSWAP
                     :
                     : "v"(a_row + ch0), "v"(a_row + ch1), "v"(w_row + ch0), "v"(w_row + ch1), "v"(voff0), "v"(voff1), "s"(base_lo), "s"(base_hi),
                       "s"(row0), "s"(lim), "s"(pitch), "s"(lds_dma), "s"(nk)
                     : UC_GLDS4_CLOBBERS);
    } else {
        asm volatile(UC_GLDS4_LOOP_SWAP
                     :
                     : "v"(a_row + ch0), "v"(a_row + ch1), "v"(w_row + ch0), "v"(w_row + ch1), "v"(voff0), "v"(voff1), "s"(base_lo), "s"(base_hi),
                       "s"(row0), "s"(lim), "s"(pitch), "s"(lds_dma), "s"(nk)
                     : UC_GLDS4_CLOBBERS);
    }
    glds_pe_t pe = *glds_kernarg_params(p);
    __builtin_amdgcn_s_barrier();          // every wave is done with the ring: it becomes the bounce space (8 KiB per wave)
    asm volatile("" ::: "memory");
    {
        float4_t acc[8][4];
        UC_GLDS4_READ_HALF0(acc)
        glds_epilogue_dispatch<8, A_MODE, EPI>(pe, acc, mode, wave_m, wave_n, tid, wave, 0, smem);
    }
    {
        float4_t acc[8][4];
        UC_GLDS4_READ_HALF1(acc)
        glds_epilogue_dispatch<8, A_MODE, EPI>(pe, acc, mode, wave_m, wave_n + 64, tid, wave, 0, smem);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// 3x3 / pad 1 / stride 1 convolution on maps at least 64 wide, ROW-WALKING form (round 3).  The implicit-GEMM kernel above stages
// a 256-pixel x 64-channel A tile per (tap, channel chunk): every input pixel crosses the LDS-DMA path nine times.  In the NT
// layout an LDS row IS a pixel, so the horizontal taps kx are ROW OFFSETS of the fragment reads: here a stage of A is the slab
// of input pixels a tile needs for ONE kernel row ky and 64 channels — for each of the tile's R = 256 / seg image-row segments the
// seg + 2 pixels ox0 - 1 .. ox0 + seg of input row oy + ky - 1 (zeros outside the image, through the descriptor's range check) — and
// the three taps (ky, 0..2) are three MFMA passes over it, each with its own 128 x 64 weight tile.  A crosses the DMA path three
// times instead of nine, with no per-tap masks; the weight tiles are what they were.
//   tile 256 pixels x 128 output channels, 8 waves of 64 x 64 (the accumulator layout of the <256, 128, 4, 2, ..> variants: the
//   shared epilogues apply unchanged); K order (ky, channel chunk, kx).
//   LDS: two slabs of 320 rows x 128 B (5 pieces per wave, the last ones may lie outside the slab: zeros) + a ring of three
//   weight tiles of 16 KiB = 128 KiB.  Unit = one (ky, chunk, kx): its weight tile, and with kx == 0 the slab; DMA two units ahead;
//   a wave waits for its own pieces of the NEXT unit only: vmcnt(2), vmcnt(2), vmcnt(7) round the three taps.
struct ConvRowsGeom {      // LDS image: slab[2] | ring of three weight tiles
    static constexpr int THREADS = 512, BM_ = 256, BN_ = 128, ROWB = 128, SLAB_ROWS = 320, SLAB_BYTES = SLAB_ROWS * ROWB, WT_BYTES = BN_ * ROWB;
    static constexpr int LDS_BYTES = 2 * SLAB_BYTES + 3 * WT_BYTES;
    static_assert(LDS_BYTES >= THREADS / 64 * GLDS_BOUNCE_BYTES, "bounce space");
};

template <int EPI, bool F16>
__global__ __launch_bounds__(ConvRowsGeom::THREADS, 2) void conv3x3_rows_kernel(GldsParams p) {
    using G = ConvRowsGeom;
    constexpr int BM_ = G::BM_, BN_ = G::BN_, ROWB = G::ROWB, SLAB_BYTES = G::SLAB_BYTES, WT_BYTES = G::WT_BYTES;
    constexpr int A_MODE = UC_A_CONV3X3, FA = 4;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int nwg = p.tiles_m * p.tiles_n;
    const int t = xcd_remap((int)blockIdx.x, nwg);
    int tm, tn;
    {   // tile order: see the 16-wave kernel
        const int GM = p.group_m;
        const int per_group = GM * p.tiles_n;
        const int grp = (int)uc_div((unsigned)t, p.dPerGroup), within = t - grp * per_group;
        const int first_m = grp * GM;
        const bool last = p.tiles_m - first_m < GM;
        const int gsz = last ? p.tiles_m - first_m : GM;
        tn = (int)uc_div((unsigned)within, last ? p.dGmLast : p.dGm);
        tm = first_m + within - tn * gsz;
    }
    const int64_t m0 = (int64_t)tm * BM_, n0 = (int64_t)tn * BN_;
    const int64_t wave_m = m0 + wr * 64, wave_n = n0 + wc * 64;

    // ---- tile geometry (wave-uniform): R row segments of seg pixels, first at (image row id rowid0 = b * H + oy0, ox0) ----
    const int W_ = p.cW, H_ = p.cH, Cin = p.cCin;
    const int seg = min(BM_, W_), R = BM_ / seg, segp = seg + 2;
    const unsigned rowid0 = uc_div((unsigned)m0, p.dWo);
    const int ox0 = (int)((unsigned)m0 - rowid0 * (unsigned)W_);
    const unsigned b0 = uc_div(rowid0, p.dHo);
    const int oy0 = (int)(rowid0 - b0 * (unsigned)H_);
    // descriptors: the slab's source window shifted back by one image row + one pixel (tap row ky and the chunk are a uniform
    // non-negative soffset), and the tile's weight rows
    const uint4_t srd_a = make_srd(p.A + (((int64_t)rowid0 - 1) * W_ + (ox0 - 1)) * Cin);
    const uint4_t srd_w = make_srd(p.W + n0 * p.K);
    // slab pieces of this wave: piece n = wave + 8 q covers slab rows 8 n .. 8 n + 7; lane -> row 8 n + lane / 8, physical chunk lane % 8
    unsigned sl_off[5], sl_mask[5];
#pragma unroll
    for (int q = 0; q < 5; ++q) {
        const int row = (wave + 8 * q) * 8 + (lane >> 3);
        const int c = (lane & 7) ^ glds_swz<64>(row);
        const int rr = row / segp, xs = row - rr * segp;             // (division by a wave-uniform value, once per tile)
        const int ix = ox0 - 1 + xs;
        sl_off[q] = (unsigned)((((int64_t)rr * W_ + xs) * Cin + c * 8) * 2);
        unsigned mask = 0;
        if (rr < R && ix >= 0 && ix < W_) {
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) mask |= ((unsigned)(oy0 + rr + ky - 1) < (unsigned)H_ ? 1u : 0u) << ky;
        }
        sl_mask[q] = mask;
    }
    unsigned w_off[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int row = (wave * 2 + q) * 8 + (lane >> 3);
        const int c = (lane & 7) ^ glds_swz<64>(row);
        w_off[q] = (unsigned)(((int64_t)row * p.K + c * 8) * 2);
    }
    const unsigned lds_base = lds_addr(smem);
    const unsigned lds_w = lds_base + 2u * SLAB_BYTES;
    const int nch = Cin / 64;
    const int nunit = 9 * nch;
    auto issue_unit = [&](int u) {                     // u = (ky * nch + chunk) * 3 + kx, wave-uniform
        const int sstep = u / 3, kx = u - 3 * sstep;
        const int ky = sstep / nch, ch = sstep - ky * nch;
        if (kx == 0) {
            const unsigned soff = (unsigned)((((int64_t)ky * W_) * Cin + ch * 64) * 2);
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                const unsigned vo = ((sl_mask[q] >> ky) & 1u) ? sl_off[q] : 0xffffffffu;
                dma16_buf_to_lds(vo, srd_a, soff, __builtin_amdgcn_readfirstlane(lds_base + (unsigned)((sstep & 1) * SLAB_BYTES + (wave + 8 * q) * 1024)));
            }
        }
        const unsigned soff_w = (unsigned)((((ky * 3 + kx) * Cin) + ch * 64) * 2);
        const int slot = u % 3;
#pragma unroll
        for (int q = 0; q < 2; ++q)
            dma16_buf_to_lds(w_off[q], srd_w, soff_w, __builtin_amdgcn_readfirstlane(lds_w + (unsigned)(slot * WT_BYTES + (wave * 2 + q) * 1024)));
    };

    // ---- fragment addressing: A fragment i of this wave = tile pixels wr * 64 + 16 i + frow = slab row base_i + frow, base_i =
    //      m_i + 2 (m_i / seg) (two halo pixels per row segment before it), + kx for the tap; W fragments as in the main kernel ----
    const int frow = lane & 15, fk = lane >> 4;
    int a_row[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int mi = wr * 64 + 16 * i;
        a_row[i] = mi + 2 * (mi / seg) + frow;
    }
    const int w_sw = glds_swz<64>(frow);
    const int w_base = (wc * 64 + frow) * ROWB;
    const int w_ch[2] = {((0 * 4 + fk) ^ w_sw) << 4, ((1 * 4 + fk) ^ w_sw) << 4};

    float4_t acc[FA][4];
#pragma unroll
    for (int i = 0; i < FA; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (float4_t){0.f, 0.f, 0.f, 0.f};

    auto compute_unit = [&](const char* slab, const char* wt, int kx) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8_t af[FA], wf[4];
#pragma unroll
            for (int i = 0; i < FA; ++i) {
                const int row = a_row[i] + kx;
                uint4 raw = *reinterpret_cast<const uint4*>(slab + row * ROWB + (((ks * 4 + fk) ^ glds_swz<64>(row)) << 4));
                if (p.relu_a) raw = relu_bf16x8(raw);
                af[i] = __builtin_bit_cast(bf16x8_t, raw);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) wf[j] = *reinterpret_cast<const bf16x8_t*>(wt + w_base + w_ch[ks] + j * 16 * ROWB);
#pragma unroll
            for (int i = 0; i < FA; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = glds_mfma<F16>(wf[j], af[i], acc[i][j]);
        }
    };

    issue_unit(0);
    if (nunit > 1) issue_unit(1);
    for (int sstep = 0; sstep < 3 * nch; ++sstep) {
        const char* slab = smem + (sstep & 1) * SLAB_BYTES;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int u = sstep * 3 + kx;
            // this wave's pieces of unit u have landed when only unit u + 1's are outstanding: 2 weight pieces (+ 5 slab pieces if
            // it opens a new slab)
            if (u + 1 >= nunit) wait_vmcnt<0>();
            else if (kx == 2) wait_vmcnt<7>();
            else wait_vmcnt<2>();
            __builtin_amdgcn_s_barrier();          // ... everyone's have; and every wave is done with unit u - 1 (its ring slot is unit u + 2's)
            asm volatile("" ::: "memory");
            if (u + 2 < nunit) issue_unit(u + 2);
            compute_unit(slab, smem + 2 * SLAB_BYTES + (u % 3) * WT_BYTES, kx);
        }
    }

    glds_pe_t pe = *glds_kernarg_params(p);
    __syncthreads();     // every wave is done with the slabs and the ring: they become the epilogue's bounce space (8 KiB per wave)
    glds_epilogue_dispatch<FA, A_MODE, EPI, F16>(pe, acc, 0, wave_m, wave_n, tid, wave, 0, smem);
}

// ---------------------------------------------------------------------------------------------------------------------------
// Eight-wave row-walking 3x3 convolution: 512 pixels x 128 output channels, 4 x 2 waves of 128 x 64 (the eight-wave GEMM's wave tile:
// 12 fragment reads feed 32 MFMAs, 384 B of LDS per MFMA against 512 B for the 64 x 64 wave tiles above), walked in 32-channel chunks.
//
//   super-step (ky, 32-channel chunk) = three units kx = 0, 1, 2 of 32 MFMAs per wave each.  Staged per super-step: the slab of input
//   pixels of kernel row ky (R row segments of seg + 2 pixels, 64-B rows: 33 pieces of 1 KiB) and the three taps' weight tiles
//   (128 x 32: 8 pieces each) — every input pixel crosses the LDS-DMA path three times, every weight tile once per 512 pixels
//   (57 KiB per super-step, 684 KiB per 512 x 128 tile at 128 input channels; the 256-pixel kernel above: 493 KiB per 256 pixels).
//   Two buffers of each (2 x 33 + 2 x 24 KiB = 114 KiB), one workgroup per CU, two waves per SIMD with 256 registers:
//
//   unit 0:  MFMAs on (a, w)   | ds_read unit 1 -> (a, wn)      (a is refilled row block by row block behind its MFMAs)
//   unit 1:  MFMAs on (a, wn)  | ds_read unit 2 -> (a, w)
//   unit 2, first four MFMA groups on (a, w)
//   s_waitcnt vmcnt(0) lgkmcnt(0) + s_barrier: everyone has READ this super-step's buffers, everyone's DMA of the next one has landed —
//            with 256 matrix-pipe cycles per wave queued, so the pipe works through the barrier's skew
//   unit 2, last four groups   | ds_read unit 0 of the next super-step -> (a, wn)
//   DMA of the super-step after the next -> the buffers just released: 7-8 pieces per wave (4-5 of the slab, 3 of the weights), one
//            behind every other MFMA group from the synchronisation to the middle of the next unit 1 (the global -> LDS path takes ~40
//            cycles per piece and CU: 57 pieces are most of a super-step; >= 1.5 units of flight each)
//
//   One barrier per 96 MFMAs of a wave.  The weight registers alternate roles from one super-step to the next (three units): the loop
//   body is a PAIR of super-steps (launcher: Cin % 64 == 0), straight-line.  Measured against the first form (synchronisation at the
//   head of unit 2, all pieces inside unit 2, a zero-writing dump piece in the odd slot of seven waves): +1-3 % (fp16 operands), level (bf16).
//   64-B LDS rows with the chunk key 3 ((row >> 2) & 1): conflict-free ds_read_b128 fragments at every row offset (the taps shift
//   the 16 rows of a fragment by kx, row segments by two halo pixels each).
//   Accumulator layout = the eight-wave GEMM's (FA = 8): the shared epilogues apply; the fused 1x1 tail drains a 128-row wave tile
//   as two 64-row halves.
//
//   FLAT (round 6): maps whose rows do NOT tile 512 pixels (148 / 296 / 592-wide: the DINOv2-518 head; 56 / 112 / 224: 224 x 224 pairs; any
//   pixel count).  A tile is 512 CONSECUTIVE output pixels of the flattened (image, y, x) order — whole or partial rows, across
//   image borders, the last tile masked by the epilogues' row bound — and the slab of kernel row ky is the 514 consecutive INPUT pixels
//   m0 + (ky - 1) W - 1 ... : tap (ky, kx) of output pixel o is input pixel o + (ky - 1) W + (kx - 1) of the same flat order, so the
//   fragment of tap kx is again the slab shifted by kx rows, with no per-segment halo.  What the flat order gets wrong is the PADDING:
//   vertically (the pixel W back / ahead of an image's first / last row belongs to the neighbouring image) the DMA zero-fills a slab
//   row whose OWN pixel (y', x') has y' - (ky - 1) outside the map — every use of that row by an existing output with the tap inside
//   its row is then right; horizontally (kx = 0 at x = 0, kx = 2 at x = W - 1 read the neighbouring ROW's edge pixel, which other
//   outputs need as it is) the fragment's lanes of those pixels are zeroed in registers.  Which of a wave's 128 pixels sit in column 0 /
//   W - 1 is wave-uniform: two 128-bit maps in 8 SGPRs (16 lane masks in SGPR pairs is more scalar state than the kernel has room for:
//   the allocator then hands an inline-asm "s" operand a VGPR); per fragment of the kx = 0 and kx = 2 units the 16-bit slice is
//   replicated over the four 16-lane groups into VCC (4 scalar instructions) and four v_cndmask_b32 zero the lanes — about what
//   the ReLU-on-load form already spends there.  (volatile: hoisted out of the loop the sixteen masks would be live SGPR pairs again.)
template <int SLICE>
__device__ __forceinline__ bf16x8_t glds_zero_edge_lanes(bf16x8_t v, unsigned map_dword) {
    uint4 q = __builtin_bit_cast(uint4, v);
    unsigned t;
    asm volatile(
        "s_bfe_u32 %4, %5, %6\n\t"
        "s_mul_i32 %4, %4, 0x10001\n\t"
        "s_mov_b32 vcc_lo, %4\n\t"
        "s_mov_b32 vcc_hi, %4\n\t"
        "v_cndmask_b32_e64 %0, %0, 0, vcc\n\t"
        "v_cndmask_b32_e64 %1, %1, 0, vcc\n\t"
        "v_cndmask_b32_e64 %2, %2, 0, vcc\n\t"
        "v_cndmask_b32_e64 %3, %3, 0, vcc"
        : "+v"(q.x), "+v"(q.y), "+v"(q.z), "+v"(q.w), "=&s"(t)
        : "s"(map_dword), "n"((16 * SLICE) | (16 << 16))
        : "vcc");
    return __builtin_bit_cast(bf16x8_t, q);
}

struct ConvRows8Geom {     // LDS image: weights[2] (three taps' tiles each) | slab[2]
    static constexpr int THREADS = 512, BM_ = 512, BN_ = 128, ROWB = 64, NPIECE = 33, SLAB_BYTES = NPIECE * 1024, WT_BYTES = 3 * BN_ * ROWB;
    static constexpr int WT0 = 0, SLAB0 = 2 * WT_BYTES, LDS_BYTES = SLAB0 + 2 * SLAB_BYTES;
    static_assert(LDS_BYTES >= THREADS / 64 * GLDS_BOUNCE_BYTES, "bounce space");
};

template <int EPI, bool F16, bool RELU_A, bool FLAT = false>
__global__ __launch_bounds__(ConvRows8Geom::THREADS, 2) void conv3x3_rows8_kernel(GldsParams p) {
    using G = ConvRows8Geom;
    constexpr int BM_ = G::BM_, BN_ = G::BN_, ROWB = G::ROWB, SLAB_BYTES = G::SLAB_BYTES, WT_BYTES = G::WT_BYTES, WT0 = G::WT0, SLAB0 = G::SLAB0;
    constexpr int A_MODE = UC_A_CONV3X3, FA = 8;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int nwg = p.tiles_m * p.tiles_n;
    const int t = xcd_remap((int)blockIdx.x, nwg);
    int tm, tn;
    {   // tile order: see the 16-wave kernel
        const int GM = p.group_m;
        const int per_group = GM * p.tiles_n;
        const int grp = (int)uc_div((unsigned)t, p.dPerGroup), within = t - grp * per_group;
        const int first_m = grp * GM;
        const bool last = p.tiles_m - first_m < GM;
        const int gsz = last ? p.tiles_m - first_m : GM;
        tn = (int)uc_div((unsigned)within, last ? p.dGmLast : p.dGm);
        tm = first_m + within - tn * gsz;
    }
    const int64_t m0 = (int64_t)tm * BM_, n0 = (int64_t)tn * BN_;
    const int64_t wave_m = m0 + wr * 128, wave_n = n0 + wc * 64;

    // ---- tile geometry (wave-uniform): R row segments of seg pixels, first at (image row id rowid0 = b * H + oy0, ox0) ----
    const int W_ = p.cW, H_ = p.cH, Cin = p.cCin;
    const int seg = FLAT ? BM_ : min(BM_, W_), R = BM_ / seg, segp = seg + 2;
    const unsigned rowid0 = uc_div((unsigned)m0, p.dWo);
    const int ox0 = (int)((unsigned)m0 - rowid0 * (unsigned)W_);
    const unsigned b0 = uc_div(rowid0, p.dHo);
    const int oy0 = (int)(rowid0 - b0 * (unsigned)H_);
    // slab row 0 of kernel row 0: segmented form = pixel (row above the tile's first, one left of its first column); flat form = flat
    // pixel m0 - W - 1.  (Either may lie before the tensor: lanes that would read there are masked — the descriptor base is only an origin.)
    const uint4_t srd_a = make_srd(FLAT ? p.A + ((int64_t)m0 - 1 - W_) * Cin : p.A + (((int64_t)rowid0 - 1) * W_ + (ox0 - 1)) * Cin);
    const uint4_t srd_w = make_srd(p.W + n0 * p.K);
    // slab pieces of this wave: piece n = wave + 8 q covers slab rows 16 n .. 16 n + 15; lane -> row 16 n + lane / 4, physical chunk lane % 4
    // (piece 32 = q 4 of wave 0 only).  sl_mask: bit 3 q + ky = the lane's pixel exists for tap row ky
    unsigned sl_off[5], sl_mask = 0;
#pragma unroll
    for (int q = 0; q < 5; ++q) {
        const int row = (wave + 8 * q) * 16 + (lane >> 2);
        const int c = (lane & 3) ^ glds_swz<32>(row);
        if constexpr (FLAT) {
            sl_off[q] = (__umul24((unsigned)row, (unsigned)Cin) + (unsigned)c * 8u) * 2u;
            asm volatile("" : "+v"(sl_off[q]));
            const int g = (int)m0 - 1 + row;                          // the slab row's own pixel (kernel row 1), flat; M < 2^30 (launcher)
            if (row < BM_ + 2 && g >= 0 && (int64_t)g < p.M && (q < 4 || wave == 0)) {
                const unsigned rid = uc_div((unsigned)g, p.dWo);      // image row id b * H + y
                const int yg = (int)(rid - uc_div(rid, p.dHo) * (unsigned)H_);
#pragma unroll
                for (int ky = 0; ky < 3; ++ky) sl_mask |= ((unsigned)(yg + ky - 1) < (unsigned)H_ ? 1u : 0u) << (3 * q + ky);
            }
        } else {
            const int rr = row / segp, xs = row - rr * segp;             // (division by a wave-uniform value, once per tile)
            const int ix = ox0 - 1 + xs;
            // (launcher: 32-bit windows, pixel and channel counts below 2^24: 24-bit multiplies — the 32-bit product of a v_mad_u64_u32
            //  lives in a register PAIR for the whole loop)
            sl_off[q] = (__umul24(__umul24((unsigned)rr, (unsigned)W_) + (unsigned)xs, (unsigned)Cin) + (unsigned)c * 8u) * 2u;
            asm volatile("" : "+v"(sl_off[q]));
            if (rr < R && ix >= 0 && ix < W_ && (q < 4 || wave == 0)) {
#pragma unroll
                for (int ky = 0; ky < 3; ++ky) sl_mask |= ((unsigned)(oy0 + rr + ky - 1) < (unsigned)H_ ? 1u : 0u) << (3 * q + ky);
            }
        }
    }
    unsigned w_off;
    {
        const int row = wave * 16 + (lane >> 2);
        const int c = (lane & 3) ^ glds_swz<32>(row);
        w_off = (__umul24((unsigned)row, (unsigned)p.K) + (unsigned)c * 8u) * 2u;
        asm volatile("" : "+v"(w_off));
    }
    const unsigned lds_base = lds_addr(smem);
    // both halves of the fifth slot's EXEC.  (Scalar by construction: as `readfirstlane(wave == 0 ? -1 : 0)` hipcc drops the readfirstlane
    //  of a value it knows to be uniform, may still SELECT it on the vector unit, and then hands the VGPR to the asm's "s" operand.)
    unsigned wave0_exec;
    asm volatile("s_cmp_eq_u32 %1, 0\n\ts_cselect_b32 %0, -1, 0" : "=s"(wave0_exec) : "s"(wave) : "scc");
    const int nch = Cin / 32;
    const int S = 3 * nch;                                   // super-steps, even (launcher)
    // piece j = 0..7 of super-step s -> buffer pair b: slab pieces q = j (j < 5), weight pieces of tap kx = j - 5
    auto issue_piece = [&](int ky, int ch, int b, int j) __attribute__((always_inline)) {
        if (j < 5) {
            // (piece 32 is wave 0's; the other waves issue their fifth slot with EXEC = 0: a branch here would split the MFMA stream into
            //  basic blocks, each join draining lgkmcnt — and accumulators spilled)
            const unsigned soff = (unsigned)((((int64_t)ky * W_) * Cin + ch * 32) * 2);
            const unsigned vo = ((sl_mask >> (3 * j + ky)) & 1u) ? sl_off[j] : 0xffffffffu;
            const unsigned dst = __builtin_amdgcn_readfirstlane(lds_base + (unsigned)(SLAB0 + b * SLAB_BYTES + (wave + 8 * j) * 1024));
            if (j == 4) dma16_buf_to_lds_if(wave0_exec, vo, srd_a, soff, dst);      // piece 32: wave 0's
            else dma16_buf_to_lds(vo, srd_a, soff, dst);
        } else {
            const int kx = j - 5;
            const unsigned soff_w = (unsigned)((((ky * 3 + kx) * Cin) + ch * 32) * 2);
            dma16_buf_to_lds(w_off, srd_w, soff_w, __builtin_amdgcn_readfirstlane(lds_base + (unsigned)(WT0 + b * WT_BYTES + kx * (BN_ * ROWB) + wave * 1024)));
        }
    };

    // ---- fragment addressing.  A fragment i of this wave = tile pixels wr * 128 + 16 i + frow = slab row mi + 2 (mi / seg) + frow + kx
    //      (two halo pixels per row segment before it); a wave's 128 pixels lie in one segment (seg >= 128): one base per tap, 16 i rows
    //      further = 1024 i bytes and the same chunk key.  W fragments: tile rows wc * 64 + 16 j + frow of the tap's 8-KiB tile ----
    const int frow = lane & 15, fk = lane >> 4;
    int a_off[3];
    {
        const int mi = wr * 128;
        const int base = mi + 2 * (mi / seg) + frow;             // (flat form: seg = 512, no halo rows between segments)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) a_off[kx] = SLAB0 + (base + kx) * ROWB + ((fk ^ glds_swz<32>(base + kx)) << 4);
    }
    // flat form: which of the wave's 128 pixels sit in column 0 / W - 1 (bit 16 i + frow of a 128-bit map; W >= 16: launcher)
    unsigned edge0[4] = {0u, 0u, 0u, 0u}, edge2[4] = {0u, 0u, 0u, 0u};
    if constexpr (FLAT) {
        const unsigned tp = (unsigned)m0 + (unsigned)(wr * 128 + frow);
        int x = (int)(tp - uc_div(tp, p.dWo) * (unsigned)W_);
#pragma unroll
        for (int i = 0; i < FA; ++i) {
            edge0[i >> 1] |= ((unsigned)__ballot(x == 0) & 0xffffu) << (16 * (i & 1));
            edge2[i >> 1] |= ((unsigned)__ballot(x == W_ - 1) & 0xffffu) << (16 * (i & 1));
            x += 16;
            if (x >= W_) x -= W_;
        }
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            edge0[d] = (unsigned)__builtin_amdgcn_readfirstlane((int)edge0[d]);
            edge2[d] = (unsigned)__builtin_amdgcn_readfirstlane((int)edge2[d]);
        }
    }
    const int w_lane = WT0 + (wc * 64 + frow) * ROWB + ((fk ^ glds_swz<32>(frow)) << 4);

    float4_t acc[FA][4];
#pragma unroll
    for (int i = 0; i < FA; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (float4_t){0.f, 0.f, 0.f, 0.f};

    bf16x8_t a[FA], w[4], wn[4];
    auto rd_a = [&](int b, int kx, int i) __attribute__((always_inline)) {
        return *reinterpret_cast<const bf16x8_t*>(smem + a_off[kx] + (b * SLAB_BYTES + i * 16 * ROWB));
    };
    auto rd_w = [&](int b, int kx, int j) __attribute__((always_inline)) {
        return *reinterpret_cast<const bf16x8_t*>(smem + w_lane + (b * WT_BYTES + kx * (BN_ * ROWB) + j * 16 * ROWB));
    };
    auto mma_row = [&](int i, bf16x8_t (&wv)[4], auto ckx) __attribute__((always_inline)) {      // ckx: the tap column these MFMAs belong to
        bf16x8_t av = a[i];
        if constexpr (RELU_A) av = __builtin_bit_cast(bf16x8_t, relu_bf16x8(__builtin_bit_cast(uint4, av)));
        if constexpr (FLAT && decltype(ckx)::value == 0) av = (i & 1) ? glds_zero_edge_lanes<1>(av, edge0[i >> 1]) : glds_zero_edge_lanes<0>(av, edge0[i >> 1]);
        if constexpr (FLAT && decltype(ckx)::value == 2) av = (i & 1) ? glds_zero_edge_lanes<1>(av, edge2[i >> 1]) : glds_zero_edge_lanes<0>(av, edge2[i >> 1]);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = glds_mfma<F16>(wv[j], av, acc[i][j]);
    };
    constexpr std::integral_constant<int, 0> KX0{};
    constexpr std::integral_constant<int, 1> KX1{};
    constexpr std::integral_constant<int, 2> KX2{};
    // one unit: MFMAs on (a, wcur) while the next unit's fragments stream into (a, wnext); the scheduling fences keep every refill of
    // a[i] behind the MFMAs that read the old a[i] (hoisted, both generations are live and the loop spills)
    auto unit = [&](bf16x8_t (&wcur)[4], bf16x8_t (&wnext)[4], int nb, int nkx, auto dma) __attribute__((always_inline)) {
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < FA; ++i) {
            if (nkx == 1) mma_row(i, wcur, KX0); else mma_row(i, wcur, KX1);      // (nkx = the tap column being LOADED: the MFMAs are one behind)
            __builtin_amdgcn_sched_barrier(0);
            if (i == 0) {
#pragma unroll
                for (int j = 0; j < 4; ++j) wnext[j] = rd_w(nb, nkx, j);
            }
            a[i] = rd_a(nb, nkx, i);
            dma(i);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    auto no_dma = [](int) __attribute__((always_inline)) {};
    auto sync = [&]() __attribute__((always_inline)) {
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    };
    // prologue: super-steps 0 and 1 -> buffers 0 and 1 back to back (both are free; loads return in order: this wave's pieces of
    // super-step 0 have landed, the second batch keeps flying under units 0 and 1)
#pragma unroll
    for (int j = 0; j < 8; ++j) issue_piece(0, 0, 0, j);
#pragma unroll
    for (int j = 0; j < 8; ++j) issue_piece(0, 1, 1, j);          // (nch >= 2: launcher)
    wait_vmcnt<7>();      // (waves 1-7 have 7 + 7 pieces in flight, wave 0 8 + 8: at most 7 outstanding = the first batch has landed)
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = rd_w(0, 0, j);
#pragma unroll
    for (int i = 0; i < FA; ++i) a[i] = rd_a(0, 0, i);
    unit(w, wn, 0, 1, no_dma);
    unit(wn, w, 0, 2, no_dma);
    // The loop is rotated so that its header sits at the synchronisation point (hipcc drains lgkmcnt at a loop header whatever is
    // pending, and there the drain is wanted).
    int ky2 = 0, ch2 = 2;                                         // (ky, chunk) of super-step s + 2, carried along
    if (ch2 >= nch) { ch2 = 0; ky2 = 1; }
    auto advance = [&]() __attribute__((always_inline)) { if (++ch2 == nch) { ch2 = 0; ++ky2; } };
    {
        // The synchronisation sits in the MIDDLE of unit 2: its first four MFMA groups (256 matrix-pipe cycles per wave, operands long in
        // registers) are queued when a wave reaches the s_waitcnt + barrier, so the pipe works through the barrier's skew instead of
        // draining behind the last fragment read; behind it the second half reads the next super-step's first fragments from the other
        // buffers; the pieces of super-step s + 2 follow one behind every other MFMA group: slots 0-1 in the rest of unit 2, 2-5 in the next
        // unit 0, 6-7 in the first half of unit 1 (>= 1.5 units of flight to the next synchronisation each).
        auto unit2a = [&](bf16x8_t (&wcur)[4]) __attribute__((always_inline)) {
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 4; ++i) mma_row(i, wcur, KX2);
            __builtin_amdgcn_sched_barrier(0);
        };
        auto unit2b = [&](bf16x8_t (&wcur)[4], bf16x8_t (&wnext)[4], int nb, auto dma) __attribute__((always_inline)) {
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < 4; ++j) wnext[j] = rd_w(nb, 0, j);
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = rd_a(nb, 0, i);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 4; i < FA; ++i) {
                mma_row(i, wcur, KX2);
                __builtin_amdgcn_sched_barrier(0);
                a[i] = rd_a(nb, 0, i);
                dma(i - 4);
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        // DMA schedule of super-step s + 2 (8 slots per wave), one piece behind every other MFMA group from the synchronisation on:
        // slots 0-1 in the rest of unit 2, 2-5 in unit 0, 6-7 in the first half of unit 1 — the global -> LDS path takes ~40 cycles
        // per piece and CU (tools/probes/dma_seg.hip): 57 pieces are 2300 of a super-step's 3072 matrix-pipe cycles, so they are spread
        // over as much of it as the buffers' release (the synchronisation) and the pieces' flight (>= 1.5 units) allow
        unit2a(w);
        for (int s = 0; s + 2 < S; s += 2) {
            sync();
            unit2b(w, wn, 1, [&](int g) __attribute__((always_inline)) { if (g & 1) issue_piece(ky2, ch2, 0, g >> 1); });                      // rest of unit 2 of s
            unit(wn, w, 1, 1, [&](int i) __attribute__((always_inline)) { if (i & 1) issue_piece(ky2, ch2, 0, 2 + (i >> 1)); });             // unit 0 of s + 1
            unit(w, wn, 1, 2, [&](int i) __attribute__((always_inline)) { if ((i & 1) && i < 4) issue_piece(ky2, ch2, 0, 6 + (i >> 1)); });  // unit 1
            advance();
            unit2a(wn);
            sync();
            unit2b(wn, w, 0, [&](int g) __attribute__((always_inline)) { if (g & 1) issue_piece(ky2, ch2, 1, g >> 1); });
            unit(w, wn, 0, 1, [&](int i) __attribute__((always_inline)) { if (i & 1) issue_piece(ky2, ch2, 1, 2 + (i >> 1)); });
            unit(wn, w, 0, 2, [&](int i) __attribute__((always_inline)) { if ((i & 1) && i < 4) issue_piece(ky2, ch2, 1, 6 + (i >> 1)); });
            advance();
            unit2a(w);
        }
        sync();
        unit2b(w, wn, 1, no_dma);
    }
    unit(wn, w, 1, 1, no_dma);
    unit(w, wn, 1, 2, no_dma);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < FA; ++i) mma_row(i, wn, KX2);

    glds_pe_t pe = *glds_kernarg_params(p);
    __syncthreads();     // every wave is done with the buffers: they become the epilogue's bounce space (8 KiB per wave)
    glds_epilogue_dispatch<FA, A_MODE, EPI, F16>(pe, acc, 0, wave_m, wave_n, tid, wave, 0, smem);
}


// ---------------------------------------------------------------------------------------------------------------------------
// Launch of a routed uc_gemm (gemm_plan.h): the plan names the kernel and its grid, the launchers below only carry it out.

// one kernel on the plan's grid with its geometry GEOM (threads, dynamic LDS bytes): tile-order fast divisions, the dynamic-LDS limit
// (set once per kernel), the launch
template <auto KFN, class GEOM>
static void glds_launch(GldsParams p, const GemmPlan& plan, hipStream_t st) {
    p.tiles_m = (int)plan.tiles_m;
    p.tiles_n = (int)plan.tiles_n;
    p.dNwg = uc_make_fastdiv((unsigned)(p.tiles_m * p.tiles_n));
    p.dPerGroup = uc_make_fastdiv((unsigned)(p.group_m * p.tiles_n));
    p.dGm = uc_make_fastdiv((unsigned)p.group_m);
    p.dGmLast = uc_make_fastdiv((unsigned)std::max(1, p.tiles_m % p.group_m));
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute((const void*)KFN, hipFuncAttributeMaxDynamicSharedMemorySize, GEOM::LDS_BYTES);
        attr_set = true;
    }
    hipLaunchKernelGGL(KFN, dim3((unsigned)p.tiles_m * (unsigned)p.tiles_n * (unsigned)plan.slices), dim3(GEOM::THREADS), GEOM::LDS_BYTES, st, p);
}

template <int BM_, int BN_, int WM_, int WN_, int STAGES, int A_MODE, int BK_, int WGS_PER_CU, int EPI, bool F16>
static void glds_launch_tile(const GldsParams& p, const GemmPlan& plan, hipStream_t st) {
    glds_launch<gemm_bf16_glds_kernel<BM_, BN_, WM_, WN_, STAGES, A_MODE, BK_, WGS_PER_CU, EPI, F16>, GldsTileGeom<BM_, BN_, WM_, WN_, STAGES, BK_>>(p, plan, st);
}

template <int EPI, bool F16, bool FLAT>
static void glds_launch_rows8(const GldsParams& p, const GemmPlan& plan, hipStream_t st) {
    if constexpr (EPI == GLDS_EPI_RES16) glds_launch<conv3x3_rows8_kernel<EPI, F16, false, FLAT>, ConvRows8Geom>(p, plan, st);   // (no ReLU on load)
    else if (plan.relu_a) glds_launch<conv3x3_rows8_kernel<EPI, F16, true, FLAT>, ConvRows8Geom>(p, plan, st);
    else glds_launch<conv3x3_rows8_kernel<EPI, F16, false, FLAT>, ConvRows8Geom>(p, plan, st);
}

// the kernels of one (A_MODE, EPI, F16) family: the eight- / four-wave and 128x64 kernels are dense bf16 only, the row-walking ones
// convolutions only, and the RES16 family has the eight-wave row kernel and the 256x256 tile
template <int A_MODE, int EPI, bool F16 = false>
static void glds_launch_family(const GldsParams& p, const GemmPlan& plan, hipStream_t st) {
    constexpr bool dense_bf16 = A_MODE == UC_A_DENSE && !F16, conv = A_MODE == UC_A_CONV3X3;
    if constexpr (EPI == GLDS_EPI_RES16) {
        switch (plan.kernel) {
            case UC_GK_CONV_ROWS8: glds_launch_rows8<EPI, F16, false>(p, plan, st); break;
            case UC_GK_CONV_ROWS8_FLAT: glds_launch_rows8<EPI, F16, true>(p, plan, st); break;
            case UC_GK_T256x256: glds_launch_tile<256, 256, 4, 4, 2, A_MODE, 64, 1, EPI, F16>(p, plan, st); break;
            default: break;
        }
    } else switch (plan.kernel) {
        case UC_GK_T128x128_S2: glds_launch_tile<128, 128, 2, 2, 2, A_MODE, 64, 1, EPI, F16>(p, plan, st); break;
        case UC_GK_T128x128_S3: glds_launch_tile<128, 128, 2, 2, 3, A_MODE, 64, 1, EPI, F16>(p, plan, st); break;
        case UC_GK_T256x128_S2: glds_launch_tile<256, 128, 4, 2, 2, A_MODE, 64, 1, EPI, F16>(p, plan, st); break;
        case UC_GK_T256x128_S3: glds_launch_tile<256, 128, 4, 2, 3, A_MODE, 64, 1, EPI, F16>(p, plan, st); break;
        case UC_GK_T256x256: glds_launch_tile<256, 256, 4, 4, 2, A_MODE, 64, 1, EPI, F16>(p, plan, st); break;
        case UC_GK_T256x128_BK32: glds_launch_tile<256, 128, 4, 2, 3, A_MODE, 32, 2, EPI, F16>(p, plan, st); break;
        case UC_GK_T128x64:
            if constexpr (dense_bf16) glds_launch_tile<128, 64, 2, 1, 3, A_MODE, 64, 1, EPI, F16>(p, plan, st);
            break;
        case UC_GK_EIGHT_WAVE:
            if constexpr (dense_bf16) glds_launch<gemm_bf16_glds8_kernel<EPI>, Glds8Geom<EPI>>(p, plan, st);
            break;
        case UC_GK_FOUR_WAVE:
            if constexpr (dense_bf16) glds_launch<gemm_bf16_glds4_kernel<EPI>, Glds4Geom>(p, plan, st);
            break;
        case UC_GK_CONV_ROWS:
            if constexpr (conv) glds_launch<conv3x3_rows_kernel<EPI, F16>, ConvRowsGeom>(p, plan, st);
            break;
        case UC_GK_CONV_ROWS8:
            if constexpr (conv) glds_launch_rows8<EPI, F16, false>(p, plan, st);
            break;
        case UC_GK_CONV_ROWS8_FLAT:
            if constexpr (conv) glds_launch_rows8<EPI, F16, true>(p, plan, st);
            break;
        default: break;
    }
}
