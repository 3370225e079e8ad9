// Eight consecutive channels of a channels-last map as one work item: one 16-byte access for the 16-bit types, two for fp32.
// Shared by the GroupNorm and the pad / crop / resize kernels (groupnorm.hip, pad_resize.hip).
#pragma once
#include "common.h"

struct NV8 { float v[8]; };

template <typename Tag> __device__ __forceinline__ NV8 nv_ld8(const typename Tag::storage* p);
template <> __device__ __forceinline__ NV8 nv_ld8<F32Tag>(const float* p) {
    NV8 r;
    const float4_t a = *reinterpret_cast<const float4_t*>(p);
    const float4_t b = *reinterpret_cast<const float4_t*>(p + 4);
    r.v[0] = a.x; r.v[1] = a.y; r.v[2] = a.z; r.v[3] = a.w; r.v[4] = b.x; r.v[5] = b.y; r.v[6] = b.z; r.v[7] = b.w;
    return r;
}
template <> __device__ __forceinline__ NV8 nv_ld8<BF16Tag>(const bf16_t* p) {
    NV8 r;
    const uint4 u = *reinterpret_cast<const uint4*>(p);
    r.v[0] = __uint_as_float(u.x << 16); r.v[1] = __uint_as_float(u.x & 0xffff0000u);
    r.v[2] = __uint_as_float(u.y << 16); r.v[3] = __uint_as_float(u.y & 0xffff0000u);
    r.v[4] = __uint_as_float(u.z << 16); r.v[5] = __uint_as_float(u.z & 0xffff0000u);
    r.v[6] = __uint_as_float(u.w << 16); r.v[7] = __uint_as_float(u.w & 0xffff0000u);
    return r;
}
template <> __device__ __forceinline__ NV8 nv_ld8<F16Tag>(const unsigned short* p) {
    NV8 r;
    const uint4 u = *reinterpret_cast<const uint4*>(p);
    const unsigned w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        r.v[2 * i] = f16_to_f32((unsigned short)(w[i] & 0xffffu));
        r.v[2 * i + 1] = f16_to_f32((unsigned short)(w[i] >> 16));
    }
    return r;
}

template <typename Tag> __device__ __forceinline__ void nv_st8(typename Tag::storage* p, const NV8& r);
template <> __device__ __forceinline__ void nv_st8<F32Tag>(float* p, const NV8& r) {
    *reinterpret_cast<float4_t*>(p) = (float4_t){r.v[0], r.v[1], r.v[2], r.v[3]};
    *reinterpret_cast<float4_t*>(p + 4) = (float4_t){r.v[4], r.v[5], r.v[6], r.v[7]};
}
template <> __device__ __forceinline__ void nv_st8<BF16Tag>(bf16_t* p, const NV8& r) {
    uint4 u;
    u.x = pack_bf16x2(r.v[0], r.v[1]); u.y = pack_bf16x2(r.v[2], r.v[3]);
    u.z = pack_bf16x2(r.v[4], r.v[5]); u.w = pack_bf16x2(r.v[6], r.v[7]);
    *reinterpret_cast<uint4*>(p) = u;
}
template <> __device__ __forceinline__ void nv_st8<F16Tag>(unsigned short* p, const NV8& r) {
    unsigned w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = (unsigned)f32_to_f16(r.v[2 * i]) | ((unsigned)f32_to_f16(r.v[2 * i + 1]) << 16);
    uint4 u;
    u.x = w[0]; u.y = w[1]; u.z = w[2]; u.w = w[3];
    *reinterpret_cast<uint4*>(p) = u;
}

// launch `kernel<Tag>` for the storage type of `dtype` (the caller has checked that dtype is one of the three)
#define NV_DISPATCH(dtype, LAUNCH)                                                  \
    do {                                                                            \
        if ((dtype) == UC_F32) { typedef F32Tag Tag; typedef float T; LAUNCH; }      \
        else if ((dtype) == UC_BF16) { typedef BF16Tag Tag; typedef bf16_t T; LAUNCH; } \
        else { typedef F16Tag Tag; typedef unsigned short T; LAUNCH; }              \
    } while (0)

static inline bool nv_dtype_ok(int dtype) { return dtype == UC_F32 || dtype == UC_BF16 || dtype == UC_F16; }
