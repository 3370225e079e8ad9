// The launch geometry and the shape rule of GroupNorm on channels-last maps (csrc/groupnorm.hip): uc_group_norm_nhwc, the SiLU entry
// points and their backward passes.
//
// Work item = 8 consecutive channels of one pixel.  A workgroup of GN_THREADS threads is laid out as `rows` pixels x C8 = C / 8 channel
// vectors (rows = GN_THREADS / C8; GN_THREADS - rows * C8 threads are dead), and takes one chunk of rows * GN_VECS pixels of one sample.
// A group is cg8 = C / G / 8 adjacent vectors, or, under the SiLU entry points, 4 channels (`half`): a vector then spans the two groups
// 2 c8 and 2 c8 + 1.  Every path reads whole vectors, so C % 8 == 0 is part of the one shape rule, groups of 4 included.
//
// Host-only, header-only and pure: no HIP header, no global state, so the system C++ compiler builds it
// (tests/groupnorm_plan_driver.cpp).  The entry points validate with gn_shape_rule, the kernels index with GnGeom and gn_group, the
// *_ws_bytes entry points size with gn_fwd_ws_bytes / gn_bwd_ws_bytes: the driver prints exactly what the device walks.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define UC_GN_HD __host__ __device__ __forceinline__
#else
#define UC_GN_HD static inline
#endif

static constexpr int GN_THREADS = 256;
static constexpr int GN_VECS = 8;            // 8-channel vectors per thread and chunk (64 values in registers)
static constexpr int GN_MAX_C = 2048;        // C / 8 <= 256: one pixel never spans more than one workgroup row

struct GnGeom {
    int HW, C, G, C8, cg8, rows, chunk_pix, nchunk;
    int cg, half;      // channels per group; half: cg == 4, the two halves of an 8-channel vector belong to groups 2 c8 and 2 c8 + 1
};
// group of half `hi` (0: channels 0..3, 1: channels 4..7) of channel vector c8
UC_GN_HD int gn_group(const GnGeom& gm, int c8, int hi) { return gm.half ? 2 * c8 + hi : c8 / gm.cg8; }

// the one shape rule, in the order the entry points report it; group4: groups of 4 channels are accepted too (the SiLU entry points)
enum GnShape { GN_SHAPE_OK = 0, GN_SHAPE_DIMS, GN_SHAPE_C_MOD_G, GN_SHAPE_GROUP, GN_SHAPE_C_MOD_8, GN_SHAPE_MAX_C, GN_SHAPE_GRID };
static inline GnShape gn_shape_rule(int64_t B, int64_t H, int64_t W, int64_t C, int64_t G, bool group4) {
    if (!(B > 0 && H > 0 && W > 0 && C > 0 && G > 0)) return GN_SHAPE_DIMS;
    if (C % G != 0) return GN_SHAPE_C_MOD_G;
    if (!((C / G) % 8 == 0 || (group4 && C / G == 4))) return GN_SHAPE_GROUP;
    if (C % 8 != 0) return GN_SHAPE_C_MOD_8;      // (groups of 4 with an odd G: a work item is 8 channels on every path)
    if (C > GN_MAX_C) return GN_SHAPE_MAX_C;
    if (!(B <= 65535 && H <= 0x7fffffff && W <= 0x7fffffff && H * W <= 0x7fffffff && B * G <= 0x7fffffff && (B * H * W * (C / 8) + 255) / 256 <= 0x7fffffff))
        return GN_SHAPE_GRID;
    return GN_SHAPE_OK;
}
static inline bool gn_shape_ok(int64_t B, int64_t H, int64_t W, int64_t C, int64_t G, bool group4) {
    return gn_shape_rule(B, H, W, C, G, group4) == GN_SHAPE_OK;
}

// a shape gn_shape_ok admits
static inline GnGeom gn_geom(int64_t H, int64_t W, int64_t C, int64_t G) {
    GnGeom g;
    g.HW = (int)(H * W);
    g.C = (int)C;
    g.G = (int)G;
    g.C8 = (int)(C / 8);
    g.cg8 = (int)(C / G / 8);
    g.cg = (int)(C / G);
    g.half = g.cg == 4;
    g.rows = GN_THREADS / g.C8;
    g.chunk_pix = g.rows * GN_VECS;
    g.nchunk = (g.HW + g.chunk_pix - 1) / g.chunk_pix;
    return g;
}

// forward workspace: (mean, M2) as two floats per (sample, chunk, group)
static inline int64_t gn_fwd_ws_bytes(int64_t B, int64_t H, int64_t W, int64_t C, int64_t G) {
    return B * (int64_t)gn_geom(H, W, C, G).nchunk * G * 8;
}
// backward workspace: part [B][nchunk][2][C], pc [B][2][C], S [B][G][2], all fp32
static inline int64_t gn_bwd_ws_bytes(int64_t B, int64_t H, int64_t W, int64_t C, int64_t G) {
    return (B * (int64_t)gn_geom(H, W, C, G).nchunk * 2 * C + B * 2 * C + B * G * 2) * 4;
}
