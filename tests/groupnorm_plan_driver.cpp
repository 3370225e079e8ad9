// CPU driver of gn_shape_rule / gn_geom / gn_fwd_ws_bytes / gn_bwd_ws_bytes (uniception_amd/csrc/groupnorm_plan.h) for
// tests/test_norm_stream_routes.py.
// stdin: one shape per line, `C G H W group4 [B]` as integers (group4: 1 = the SiLU entry points' rule; B defaults to 2).
// stdout, one line per shape: `ok C8 cg8 half rows chunk_pix nchunk dead_threads fwd_ws_bytes bwd_ws_bytes`, or `refused`.
#include <stdio.h>
#include "groupnorm_plan.h"

int main() {
    char line[512];
    while (fgets(line, sizeof line, stdin)) {
        long long C, G, H, W, g4, B = 2;
        const int n = sscanf(line, "%lld %lld %lld %lld %lld %lld", &C, &G, &H, &W, &g4, &B);
        if (n < 5) {
            fprintf(stderr, "bad row %s", line);
            return 2;
        }
        if (!gn_shape_ok(B, H, W, C, G, g4 != 0)) {
            printf("refused\n");
            continue;
        }
        const GnGeom gm = gn_geom(H, W, C, G);
        // gn_group over every vector stays inside [0, G): the kernels index mean / rstd / S with it
        for (int c8 = 0; c8 < gm.C8; ++c8)
            for (int hi = 0; hi < 2; ++hi)
                if (gn_group(gm, c8, hi) < 0 || gn_group(gm, c8, hi) >= gm.G) {
                    fprintf(stderr, "group out of range\n");
                    return 3;
                }
        printf("ok %d %d %d %d %d %d %d %lld %lld\n", gm.C8, gm.cg8, gm.half, gm.rows, gm.chunk_pix, gm.nchunk, GN_THREADS - gm.rows * gm.C8,
               (long long)gn_fwd_ws_bytes(B, H, W, C, G), (long long)gn_bwd_ws_bytes(B, H, W, C, G));
    }
    return 0;
}
