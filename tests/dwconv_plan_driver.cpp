// CPU driver of uc_dwconv_plan / uc_dwconv_wgrad_plan (uniception_amd/csrc/dwconv_plan.h) for tests/test_dinov3_convnext.py.
// stdin: one launch per line, `name=value` tokens: op (fwd | wgrad), dtype (0 f32, 1 bf16, 2 f16), B, H, W, C.
// The driver WALKS the plan the way the kernels of csrc/dwconv.hip do — every workgroup, every work item, through the same decode
// functions and the same guards — and counts how often each output is produced and whether every LDS index stays inside the bytes
// the plan states.
// stdout, one line per launch:
//   fwd   tile_h tile_w c8 pix_stride chunks tiles_y tiles_x items threads lds_in_bytes lds_w_bytes lds_bytes grid cover_min cover_max lds_ok
//         (cover: over all outputs (b, y, x, 8-channel vector), how many work items store it)
//   wgrad tile_h tile_w c8 pix_stride chunks tiles_y tiles_x row_groups threads lds_x_bytes lds_dy_bytes lds_red_bytes lds_bytes units
//         partials merge_depth ws_bytes cover_min cover_max lds_ok ws_ok
//         (cover: over all (b, y, x, ky, 8-channel vector), how many work items add that dy pixel into their tap row; ws_ok: every
//         partial a workgroup writes lies inside ws_bytes)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "dwconv_plan.h"

struct Launch { int op; long long dtype, B, H, W, C; };

static bool set_field(Launch& l, const std::string& n, const char* v) {
    if (n == "op") {
        l.op = !strcmp(v, "fwd") ? 0 : !strcmp(v, "wgrad") ? 1 : -1;
        return l.op >= 0;
    }
    const long long i = strtoll(v, nullptr, 0);
#define I(f) if (n == #f) { l.f = i; return true; }
    I(dtype) I(B) I(H) I(W) I(C)
#undef I
    return false;
}

static void walk_fwd(const Launch& l) {
    const int B = (int)l.B, H = (int)l.H, W = (int)l.W, C = (int)l.C, C8 = C / 8;
    const DwconvPlan p = uc_dwconv_plan((int)l.dtype, B, H, W, C);
    std::vector<int> cover((size_t)B * H * W * C8, 0);
    bool lds_ok = p.lds_bytes == p.lds_in_bytes + p.lds_w_bytes && p.items <= p.threads && p.threads <= UC_DW_MAX_THREADS && p.threads % 64 == 0;
    const int lw = p.tile_w + 2 * UC_DW_RADIUS, lh = p.tile_h + 2 * UC_DW_RADIUS;
    // the staging loop's last vector and the weights' last vector end inside their regions
    lds_ok = lds_ok && ((long long)(lh * lw - 1) * p.pix_stride + p.c8) * p.vec_bytes <= p.lds_in_bytes && UC_DW_TAPS * p.c8 * 32 <= p.lds_w_bytes;
    for (int64_t blk = 0; blk < p.grid; ++blk) {
        const DwconvBlock k = uc_dwconv_block(p.tiles_x, p.tiles_y, p.chunks, blk);
        for (int it = 0; it < p.items; ++it) {
            const DwconvItem m = uc_dwconv_item(p.c8, p.tile_w, it);
            const int gc8 = k.chunk * p.c8 + m.c8, gy = k.ty * p.tile_h + m.row, gx0 = k.tx * p.tile_w + m.run * UC_DW_RUN;
            if (gc8 >= C8 || gy >= H || gx0 >= W) continue;
            // the farthest vector this item reads: row + 6, column run * 4 + 9
            const long long last = ((long long)(m.row + 6) * lw + m.run * UC_DW_RUN + UC_DW_RUN + 5) * p.pix_stride + m.c8;
            lds_ok = lds_ok && (last + 1) * p.vec_bytes <= p.lds_in_bytes && k.b < B;
            for (int r = 0; r < UC_DW_RUN; ++r)
                if (gx0 + r < W) ++cover[(((size_t)k.b * H + gy) * W + gx0 + r) * C8 + gc8];
        }
    }
    int lo = 1 << 30, hi = 0;
    for (int c : cover) { lo = c < lo ? c : lo; hi = c > hi ? c : hi; }
    printf("fwd %d %d %d %d %d %d %d %d %d %d %d %d %lld %d %d %d\n", p.tile_h, p.tile_w, p.c8, p.pix_stride, p.chunks, p.tiles_y, p.tiles_x, p.items,
           p.threads, p.lds_in_bytes, p.lds_w_bytes, p.lds_bytes, (long long)p.grid, lo, hi, (int)lds_ok);
}

static void walk_wgrad(const Launch& l) {
    const int B = (int)l.B, H = (int)l.H, W = (int)l.W, C = (int)l.C, C8 = C / 8;
    const DwconvWgradPlan p = uc_dwconv_wgrad_plan((int)l.dtype, B, H, W, C);
    std::vector<int> cover((size_t)B * H * W * 7 * C8, 0);
    const int lw = p.tile_w + 2 * UC_DW_RADIUS, lh = p.tile_h + 2 * UC_DW_RADIUS;
    bool lds_ok = p.lds_bytes == p.lds_x_bytes + p.lds_dy_bytes + p.lds_red_bytes && p.threads <= UC_DW_MAX_THREADS && p.threads % 64 == 0 &&
                  7 * p.c8 * p.row_groups <= p.threads && p.partials >= 1 && p.partials <= p.units;
    lds_ok = lds_ok && ((long long)(lh * lw - 1) * p.pix_stride + p.c8) * p.vec_bytes <= p.lds_x_bytes &&
             ((long long)(p.tile_h * p.tile_w - 1) * p.pix_stride + p.c8) * p.vec_bytes <= p.lds_dy_bytes && UC_DW_WS_ROWS * p.c8 * 32 <= p.lds_red_bytes;
    bool ws_ok = p.ws_bytes == (int64_t)p.partials * UC_DW_WS_ROWS * C * 4;
    for (int chunk = 0; chunk < p.chunks; ++chunk)
        for (int part = 0; part < p.partials; ++part) {
            for (int tid = 0; tid < p.threads; ++tid) {
                const DwconvWgradItem m = uc_dwconv_wgrad_item(p.c8, tid);
                const int gc8 = chunk * p.c8 + m.c8;
                if (!(m.group < p.row_groups && gc8 < C8)) continue;
                if (m.group == 0)       // this item writes rows ky * 7 .. + 6 (and 49) of partial `part`, 8 floats at column gc8 * 8
                    ws_ok = ws_ok && ((int64_t)part * UC_DW_WS_ROWS * C + (int64_t)UC_DW_TAPS * C + gc8 * 8 + 8) * 4 <= p.ws_bytes;
                for (int64_t u = part; u < p.units; u += p.partials) {
                    const int tx = (int)(u % p.tiles_x), ty = (int)((u / p.tiles_x) % p.tiles_y);
                    const int64_t b = u / ((int64_t)p.tiles_x * p.tiles_y);
                    for (int row = m.group; row < p.tile_h; row += p.row_groups)
                        for (int j = 0; j < p.tile_w; ++j) {
                            const int gy = ty * p.tile_h + row, gx = tx * p.tile_w + j;
                            lds_ok = lds_ok && (((long long)(row + m.ky) * lw + j + 6) * p.pix_stride + m.c8 + 1) * p.vec_bytes <= p.lds_x_bytes;
                            if (gy < H && gx < W && b < B) ++cover[((((size_t)b * H + gy) * W + gx) * 7 + m.ky) * C8 + gc8];
                        }
                }
            }
        }
    int lo = 1 << 30, hi = 0;
    for (int c : cover) { lo = c < lo ? c : lo; hi = c > hi ? c : hi; }
    printf("wgrad %d %d %d %d %d %d %d %d %d %d %d %d %d %lld %d %d %lld %d %d %d %d\n", p.tile_h, p.tile_w, p.c8, p.pix_stride, p.chunks, p.tiles_y,
           p.tiles_x, p.row_groups, p.threads, p.lds_x_bytes, p.lds_dy_bytes, p.lds_red_bytes, p.lds_bytes, (long long)p.units, p.partials,
           p.merge_depth, (long long)p.ws_bytes, lo, hi, (int)lds_ok, (int)ws_ok);
}

int main() {
    char line[4096];
    while (fgets(line, sizeof line, stdin)) {
        Launch l;
        memset(&l, 0, sizeof l);
        l.op = -1;
        for (char* t = strtok(line, " \t\n"); t; t = strtok(nullptr, " \t\n")) {
            char* eq = strchr(t, '=');
            if (!eq || !set_field(l, std::string(t, eq - t), eq + 1)) {
                fprintf(stderr, "bad token %s\n", t);
                return 2;
            }
        }
        if (l.op < 0 || l.B <= 0 || l.H <= 0 || l.W <= 0 || l.C <= 0 || l.C % 8) {
            fprintf(stderr, "bad launch\n");
            return 2;
        }
        if (l.op == 0) walk_fwd(l);
        else walk_wgrad(l);
    }
    return 0;
}
