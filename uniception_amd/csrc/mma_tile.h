// What the tiled MFMA kernels (GEMMs, attention forward and backward) share: operand vector types, the swizzled LDS tile image, the
// asynchronous global -> LDS copy (LDS-DMA) with its buffer descriptor, the XCD-aware workgroup orders, the packed-bf16 ReLU and
// the transposing LDS read.  Each of them exists ONCE, here.
#pragma once
#include "common.h"

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));      // one MFMA operand of the x32 (16x16) / x16 (32x32) bf16 instructions
typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));      // what one transposing LDS read returns
typedef bf16x2v_t bf16x2_t;
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
typedef unsigned uint4_t __attribute__((ext_vector_type(4)));     // a buffer descriptor (four SGPRs)
typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef __attribute__((address_space(3))) bf16x4_t* lds_v4_t;

// 32-bit LDS byte address of a __shared__ object: what M0 and the DMA destinations are computed from
__device__ __forceinline__ unsigned lds_addr(const void* smem) { return (unsigned)(size_t)(lds_ptr_t)smem; }

// Byte offset of 16-byte chunk `chunk` of row `row` in a tile of 64-channel bf16 rows (128 B per row).  The chunk index is XOR-ed with
// (row >> 1) & 7, which makes the ds_read_b128 fragment loads (lane = row, lane >> 4 = k chunk) conflict-free inside the hardware's
// 16-lane service groups.  The DMA writes lane-linear, so the same involution is applied to its per-lane SOURCE address: the two must
// agree, which is why there is one definition.  tile_swz_chunk is the offset inside the row, for the one caller (tr_operand) whose
// address has to stay a chain of pointer additions: summed as an int first, its kernels schedule differently.
__device__ __forceinline__ int tile_swz_chunk(int row, int chunk) { return (chunk ^ ((row >> 1) & 7)) << 4; }
__device__ __forceinline__ int tile_swz(int row, int chunk) { return row * 128 + tile_swz_chunk(row, chunk); }

// key offset inside a 16-key group for VT position pp (inverse of uc_vt_perm, include/uc_hip.h)
__device__ __forceinline__ int vt_key_of_pos(int pp) {
    const int hi = pp >> 3, j = pp & 7;
    return (j & 3) + 8 * (j >> 2) + 4 * hi;
}

// ---------------------------------------------------------------------------------------------------------------------------
// LDS-DMA: one wave-instruction copies 64 lanes x 16 B (1 KiB) from global memory to LDS at M0 + lane * 16, no VGPR in between.
// Issued through inline asm: with the __builtin form hipcc tracks the DMA as an LDS write it cannot disambiguate from the fragment
// ds_reads of the OTHER stage buffer and inserts `s_waitcnt vmcnt(0)` in front of them — the whole global->LDS latency is then
// exposed in every K-step (measured: matrix pipe 39 % busy, 57 % of wave cycles parked).  The asm form is invisible to that pass;
// completion is enforced by hand with counted wait_vmcnt<N>() + s_barrier (see the K-loops).
// M0 carries the wave-uniform LDS byte address.  It is compiler-reserved, so it is saved and restored inside the statement — except
// in the b64_* forms, which declare it clobbered.  Nops: s_nop 0 covers the M0-write -> LDS-DMA hazard of the global forms, whose
// other operands are VGPRs or long-lived SGPRs; the buffer forms take a descriptor / soffset that may have been written by the
// preceding scalar instructions, and s_nop 4 covers SGPR write -> VMEM read as well.
// ---------------------------------------------------------------------------------------------------------------------------
// global form: 64-bit per-lane address
__device__ __forceinline__ void dma16_to_lds(const void* gsrc, unsigned lds_byte_addr) {
    unsigned keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %2\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %1, off\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(gsrc), "s"(lds_byte_addr)
        : "memory");
}
// saddr form: wave-uniform 64-bit base (SGPR pair) + 32-bit per-lane byte offset
__device__ __forceinline__ void dma16_s_to_lds(unsigned voff, const void* sbase, unsigned lds_byte_addr) {
    unsigned keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %3\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %1, %2\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(voff), "s"(sbase), "s"(lds_byte_addr)
        : "memory");
}
// buffer form: source = descriptor base + voff + soff (bytes); a lane whose offset is outside the descriptor's range gets zeros
// written to its 16 LDS bytes
__device__ __forceinline__ void dma16_buf_to_lds(unsigned voff, uint4_t srd, unsigned soff, unsigned lds_byte_addr) {
    unsigned keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %3\n\t"
        "s_nop 4\n\t"
        "buffer_load_dwordx4 %1, %2, %4 offen lds\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(voff), "s"(srd), "s"(lds_byte_addr), "s"(soff)
        : "memory");
}
// ... under a wave-uniform execution mask (all lanes or none): a slot of a fixed per-wave DMA schedule that only some waves fill is
// issued with EXEC = 0 by the others — no branch in the instruction stream (a branch splits the MFMA stream into basic blocks),
// no work in the memory pipeline.
__device__ __forceinline__ void dma16_buf_to_lds_if(unsigned exec_half, unsigned voff, uint4_t srd, unsigned soff, unsigned lds_byte_addr) {
    unsigned keep;
    unsigned long long keep_exec;
    asm volatile(
        "s_mov_b64 %0, exec\n\t"
        "s_mov_b32 %1, m0\n\t"
        "s_mov_b32 m0, %4\n\t"
        "s_mov_b32 exec_lo, %6\n\t"
        "s_mov_b32 exec_hi, %6\n\t"
        "s_nop 4\n\t"
        "buffer_load_dwordx4 %2, %3, %5 offen lds\n\t"
        "s_mov_b64 exec, %0\n\t"
        "s_mov_b32 m0, %1"
        : "=&s"(keep_exec), "=&s"(keep)
        : "v"(voff), "s"(srd), "s"(lds_byte_addr), "s"(soff), "s"(exec_half)
        : "memory");
}
// buffer forms with M0 declared clobbered, for the one-wave-per-SIMD backward kernels: every instruction is four cycles of the wave's
// issue time there, and the save / restore pair of dma16_buf_to_lds is two of five.  b64_dma4: 64 lanes x 4 B.
__device__ __forceinline__ void b64_dma16(unsigned voff, uint4_t srd, unsigned soff, unsigned lds_byte_addr) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, %3 offen lds" : : "v"(voff), "s"(srd), "s"(lds_byte_addr), "s"(soff) : "memory", "m0");
}
__device__ __forceinline__ void b64_dma4(unsigned voff, uint4_t srd, unsigned soff, unsigned lds_byte_addr) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dword %0, %1, %3 offen lds" : : "v"(voff), "s"(srd), "s"(lds_byte_addr), "s"(soff) : "memory", "m0");
}
template <int N_>
__device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N_) : "memory"); }

// Buffer descriptor of `bytes` bytes from `base` (raw buffer, stride 0; word 3 = 0x00020000: 32-bit data format, offsets beyond
// `bytes` read as zeros), wave-uniform by readfirstlane.  The default size is "everything": callers that need the range check set one.
__device__ __forceinline__ uint4_t make_srd(const void* base, unsigned bytes = 0xffffff00u) {
    const unsigned long long pa = (unsigned long long)base;
    return (uint4_t){(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)pa),
                     (unsigned)__builtin_amdgcn_readfirstlane((int)((unsigned)(pa >> 32) & 0xffffu)),
                     (unsigned)__builtin_amdgcn_readfirstlane((int)bytes), 0x00020000u};
}

// XCD-aware orders.  Workgroup w runs on XCD w % 8 (round-robin dispatch), each XCD with its own L2.
// GEMMs: give each XCD a contiguous run of tiles, so that tiles which share an A row-panel / W column-panel share one L2.
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
    const int q = nwg >> 3, r = nwg & 7;
    const int xcd = bid & 7, k = bid >> 3;
    const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + k;
}
// Attention, 1-D grid -> (tile, batch * head): the nt tiles that share one (batch, head)'s operands get ids that differ by multiples
// of 8 and meet in ONE XCD's L2 instead of pulling the same rows through all eight.  Whole groups of 8 (batch, head) pairs; the
// last, partial group runs in plain order.
__device__ __forceinline__ void xcd_tile_order(int w, int nt, int nbh, int& tile, int& bh) {
    const int per_group = 8 * nt;
    const int grp = w / per_group, within = w - grp * per_group;
    if ((grp + 1) * 8 <= nbh) { bh = grp * 8 + (within & 7); tile = within >> 3; }
    else { const int rem = w - (nbh / 8) * 8 * nt; bh = (nbh / 8) * 8 + rem / nt; tile = rem % nt; }
}
// ... with the host's exact fast divisions by 8 * nt (dGroup) and nt (dNq)
__device__ __forceinline__ void xcd_tile_order(int w, int nt, int nbh, uc_fastdiv dGroup, uc_fastdiv dNq, int& tile, int& bh) {
    const int per_group = 8 * nt;
    const int grp = (int)uc_div((unsigned)w, dGroup), within = w - grp * per_group;
    if ((grp + 1) * 8 <= nbh) { bh = grp * 8 + (within & 7); tile = within >> 3; }
    else {
        const int rem = w - (nbh >> 3) * 8 * nt, rb = (int)uc_div((unsigned)rem, dNq);
        bh = (nbh >> 3) * 8 + rb; tile = rem - rb * nt;
    }
}

// ReLU of packed bf16: a bf16 is negative exactly when its bit pattern is negative as an int16, so max(int16, 0) is the ReLU
// (-0 -> +0): one v_pk_max_i16 per register instead of shift / and / multiply / and-not — the fragment-load ReLU of the residual
// conv units sits in the K-loop, where vector instructions take their cycles from the matrix pipe.
typedef short short2v_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint4 relu_bf16x8(uint4 v) {
    unsigned* q = reinterpret_cast<unsigned*>(&v);
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] = __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(short2v_t, q[i]), (short2v_t){0, 0}));
    return v;
}
__device__ __forceinline__ bf16x4_t relu_bf16x4(bf16x4_t v) {
    uint2 u = __builtin_bit_cast(uint2, v);
    unsigned* q = reinterpret_cast<unsigned*>(&u);
#pragma unroll
    for (int i = 0; i < 2; ++i) q[i] = __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(short2v_t, q[i]), (short2v_t){0, 0}));
    return __builtin_bit_cast(bf16x4_t, u);
}

// One transposing 8-byte LDS read (ds_read_b64_tr_b16): a 16-lane group hands in the addresses of four rows of 16 bf16 (lane q: 4
// consecutive bf16 of row q >> 2) and receives, per lane, column q of that 4 x 16 block.  Two of them make one MFMA operand.
__device__ __forceinline__ bf16x4_t lds_read_tr16(const char* p) { return __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_v4_t)(lds_ptr_t)p); }
