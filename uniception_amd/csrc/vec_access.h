// What the streaming (HBM-bound) kernels share: N consecutive elements of one storage type <-> fp32 registers, the capped
// grid-stride grid, and the run-time dtype -> Tag dispatch of the extern "C" entry points.
//   Vec8  / vec_load8 / vec_store8 : eight consecutive channels of a channels-last map as one work item — one 16-byte access for the
//                                    16-bit types, two for fp32 (F32Tag, BF16Tag, F16Tag)
//   float4_t / vec_load4 / vec_store4 : four consecutive elements, 16 bytes of fp32 or 8 of bf16 (F32Tag, BF16Tag)
#pragma once
#include "common.h"
#include "stream_plan.h"

struct Vec8 { float v[8]; };

__device__ __forceinline__ unsigned pack_f16x2(float lo, float hi) {       // round-to-nearest-even, like torch's Half
    const float2v_t v = {uc_sat_f16(lo), uc_sat_f16(hi)};            // (saturating: see common.h)
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, half2v_t));
}
__device__ __forceinline__ void unpack_f16x2(unsigned u, float& lo, float& hi) {
    const float2v_t v = __builtin_convertvector(__builtin_bit_cast(half2v_t, u), float2v_t);
    lo = v.x; hi = v.y;
}
// four bf16 as they lie in memory -> fp32 (bf16 -> fp32 is a shift: common.h)
__device__ __forceinline__ float4_t unpack_bf16x4(uint2 r) {
    return (float4_t){__uint_as_float(r.x << 16), __uint_as_float(r.x & 0xffff0000u), __uint_as_float(r.y << 16), __uint_as_float(r.y & 0xffff0000u)};
}

template <typename Tag> __device__ __forceinline__ Vec8 vec_load8(const typename Tag::storage* p);
template <> __device__ __forceinline__ Vec8 vec_load8<F32Tag>(const float* p) {
    Vec8 r;
    const float4_t a = *reinterpret_cast<const float4_t*>(p);
    const float4_t b = *reinterpret_cast<const float4_t*>(p + 4);
    r.v[0] = a.x; r.v[1] = a.y; r.v[2] = a.z; r.v[3] = a.w; r.v[4] = b.x; r.v[5] = b.y; r.v[6] = b.z; r.v[7] = b.w;
    return r;
}
template <> __device__ __forceinline__ Vec8 vec_load8<BF16Tag>(const bf16_t* p) {
    Vec8 r;
    const uint4 u = *reinterpret_cast<const uint4*>(p);
    r.v[0] = __uint_as_float(u.x << 16); r.v[1] = __uint_as_float(u.x & 0xffff0000u);
    r.v[2] = __uint_as_float(u.y << 16); r.v[3] = __uint_as_float(u.y & 0xffff0000u);
    r.v[4] = __uint_as_float(u.z << 16); r.v[5] = __uint_as_float(u.z & 0xffff0000u);
    r.v[6] = __uint_as_float(u.w << 16); r.v[7] = __uint_as_float(u.w & 0xffff0000u);
    return r;
}
template <> __device__ __forceinline__ Vec8 vec_load8<F16Tag>(const unsigned short* p) {
    Vec8 r;
    const uint4 u = *reinterpret_cast<const uint4*>(p);
    unpack_f16x2(u.x, r.v[0], r.v[1]); unpack_f16x2(u.y, r.v[2], r.v[3]);
    unpack_f16x2(u.z, r.v[4], r.v[5]); unpack_f16x2(u.w, r.v[6], r.v[7]);
    return r;
}

template <typename Tag> __device__ __forceinline__ void vec_store8(typename Tag::storage* p, const Vec8& r);
template <> __device__ __forceinline__ void vec_store8<F32Tag>(float* p, const Vec8& r) {
    *reinterpret_cast<float4_t*>(p) = (float4_t){r.v[0], r.v[1], r.v[2], r.v[3]};
    *reinterpret_cast<float4_t*>(p + 4) = (float4_t){r.v[4], r.v[5], r.v[6], r.v[7]};
}
template <> __device__ __forceinline__ void vec_store8<BF16Tag>(bf16_t* p, const Vec8& r) {
    uint4 u;
    u.x = pack_bf16x2(r.v[0], r.v[1]); u.y = pack_bf16x2(r.v[2], r.v[3]);
    u.z = pack_bf16x2(r.v[4], r.v[5]); u.w = pack_bf16x2(r.v[6], r.v[7]);
    *reinterpret_cast<uint4*>(p) = u;
}
template <> __device__ __forceinline__ void vec_store8<F16Tag>(unsigned short* p, const Vec8& r) {
    uint4 u;
    u.x = pack_f16x2(r.v[0], r.v[1]); u.y = pack_f16x2(r.v[2], r.v[3]);
    u.z = pack_f16x2(r.v[4], r.v[5]); u.w = pack_f16x2(r.v[6], r.v[7]);
    *reinterpret_cast<uint4*>(p) = u;
}

template <typename Tag> __device__ __forceinline__ float4_t vec_load4(const typename Tag::storage* p);
template <> __device__ __forceinline__ float4_t vec_load4<F32Tag>(const float* p) { return *reinterpret_cast<const float4_t*>(p); }
template <> __device__ __forceinline__ float4_t vec_load4<BF16Tag>(const bf16_t* p) { return unpack_bf16x4(*reinterpret_cast<const uint2*>(p)); }

template <typename Tag> __device__ __forceinline__ void vec_store4(typename Tag::storage* p, float4_t v);
template <> __device__ __forceinline__ void vec_store4<F32Tag>(float* p, float4_t v) { *reinterpret_cast<float4_t*>(p) = v; }
template <> __device__ __forceinline__ void vec_store4<BF16Tag>(bf16_t* p, float4_t v) {
    *reinterpret_cast<uint2*>(p) = (uint2){pack_bf16x2(v.x, v.y), pack_bf16x2(v.z, v.w)};
}

// grid of a grid-stride kernel with 256-thread workgroups (the cap: stream_plan.h)
#define EW_GRID(n_items) uc_stream_grid((n_items), UC_STREAM_WG, UC_EW_GRID_CAP)

// ---- one storage dtype chosen at run time ----------------------------------------------------------------------------------------
// An entry point accepts {UC_F32, UC_BF16} (UC_DISPATCH) or {UC_F32, UC_BF16, UC_F16} (UC_DISPATCH_F16); which of the two is written
// at the call site, so a kernel is instantiated for exactly the tags its entry point accepts.  LAUNCH is the launch, written once
// with `Tag` (pointers are cast to Tag::storage); any other code is rejected with UC_ERR_BAD_ARG before LAUNCH runs.
// UC_REQUIRE_DTYPE is the same check on its own, for entry points that look at the dtype before their shape checks.
#define UC_REQUIRE_DTYPE(fn, dtype, F16)                                                                                    \
    UC_REQUIRE((dtype) == UC_F32 || (dtype) == UC_BF16 || ((F16) && (dtype) == UC_F16), "%s: unsupported dtype %d (%s)", fn, \
               dtype, (F16) ? "UC_F32, UC_BF16 or UC_F16" : "UC_F32 or UC_BF16")
#define UC_DISPATCH(fn, dtype, LAUNCH)                                              \
    do {                                                                            \
        UC_REQUIRE_DTYPE(fn, dtype, false);                                         \
        if ((dtype) == UC_F32) { typedef F32Tag Tag; LAUNCH; }                      \
        else { typedef BF16Tag Tag; LAUNCH; }                                       \
    } while (0)
#define UC_DISPATCH_F16(fn, dtype, LAUNCH)                                          \
    do {                                                                            \
        UC_REQUIRE_DTYPE(fn, dtype, true);                                          \
        if ((dtype) == UC_F32) { typedef F32Tag Tag; LAUNCH; }                      \
        else if ((dtype) == UC_BF16) { typedef BF16Tag Tag; LAUNCH; }               \
        else { typedef F16Tag Tag; LAUNCH; }                                        \
    } while (0)
