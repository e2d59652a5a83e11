// The per-edge arithmetic of the polygon rasteriser (pycocotools' rleFrPoly restated per crossing: poly_rle.hip's header comment, DESIGN.md
// section 20), shared by afi_poly_rle_count (poly_rle.hip) and afi_mask_targets (mask_loss.hip): an edge's upsampled end points, its walking
// order, its candidate columns and the crossing of one candidate.
#pragma once

struct PolyEdge { int xs, ys, xe, ye; };               // upsampled, in the polygon's order

// Every fp64 step below is one rounded operation: plain operators under `fp contract(off)` (hipcc's __dmul_rn / __dadd_rn are header
// functions whose product and sum it still fuses; tests/test_gpu_poly.py holds polygons that a fused step 2 rasterises differently).

__device__ __forceinline__ int poly_up(double c) {
#pragma clang fp contract(off)
    const double m = 5.0 * c;
    return (int)(m + 0.5);
}

// (int)(b + s t + .5): a rounded product and two rounded sums
__device__ __forceinline__ int poly_at(int b, double s, int t) {
#pragma clang fp contract(off)
    const double m = s * (double)t;
    const double a = (double)b + m;
    return (int)(a + 0.5);
}

// The edge in walking order: flip, the end points after the swap, the slope and the length in points - 1.
struct PolyWalk { int xs, ys, L; double s; bool xmajor, flip; };

__device__ __forceinline__ PolyWalk poly_walk(const PolyEdge& e) {
#pragma clang fp contract(off)
    PolyWalk w;
    const long long ddx = (long long)e.xe - e.xs, ddy = (long long)e.ye - e.ys;
    const int dx = (int)(ddx < 0 ? -ddx : ddx), dy = (int)(ddy < 0 ? -ddy : ddy);      // < 2^31: |coordinate| < 2^30
    w.xmajor = dx >= dy;
    w.flip = (w.xmajor && e.xs > e.xe) || (!w.xmajor && e.ys > e.ye);
    w.xs = w.flip ? e.xe : e.xs;
    w.ys = w.flip ? e.ye : e.ys;
    const int xe = w.flip ? e.xs : e.xe, ye = w.flip ? e.ys : e.ye;
    w.L = w.xmajor ? dx : dy;
    w.s = 0.0;
    if (w.L > 0) w.s = w.xmajor ? (double)(ye - w.ys) / (double)dx : (double)(xe - w.xs) / (double)dy;
    return w;
}

// The candidate columns q of an edge: qlo .. qlo + n - 1.
__device__ __forceinline__ int poly_edge_cands(const PolyEdge& e, int W, int* qlo) {
    const PolyWalk w = poly_walk(e);
    *qlo = 0;
    if (w.L == 0) return 0;
    int ua, ub;
    if (w.xmajor) {
        ua = w.xs;
        ub = w.xs + w.L;
    } else {
        if (e.xs == e.xe) return 0;                     // s = 0: one column
        ua = poly_at(w.xs, w.s, 0);
        ub = poly_at(w.xs, w.s, w.L);
    }
    const int umin = ua < ub ? ua : ub, umax = ua < ub ? ub : ua;
    if (umax < 3) return 0;                             // c = 5 q + 2 <= umax - 1 with q >= 0
    const int lo = umin <= 2 ? 0 : (umin + 2) / 5;      // ceil((umin - 2) / 5)
    int hi = (umax - 3) / 5;
    if (hi > W - 1) hi = W - 1;
    *qlo = lo;
    return hi >= lo ? hi - lo + 1 : 0;
}

// The crossing a of candidate column q of an edge (H W: no crossing of the reference at this candidate; dropped with the crossings at H W).
__device__ __forceinline__ int poly_crossing(const PolyEdge& e, int q, int H, int HW) {
#pragma clang fp contract(off)
    const PolyWalk w = poly_walk(e);
    const int c = 5 * q + 2;
    int ymin;
    if (w.xmajor) {
        const int t0 = c - w.xs;
        const int v0 = poly_at(w.ys, w.s, t0), v1 = poly_at(w.ys, w.s, t0 + 1);
        ymin = v0 < v1 ? v0 : v1;
    } else {
        const bool up = w.s > 0.0;                      // the column rises with t
        int lo = 0, hi = w.L;                           // up: u(lo) <= c < u(hi); down: u(lo) > c >= u(hi)
        while (hi - lo > 1) {
            const int mid = lo + ((hi - lo) >> 1);
            const int u = poly_at(w.xs, w.s, mid);
            if ((u > c) == up) hi = mid; else lo = mid;
        }
        const int u_lo = poly_at(w.xs, w.s, lo), u_hi = poly_at(w.xs, w.s, hi);
        const bool rising = up != w.flip;               // in the polygon's order
        const int upper = up ? u_hi : u_lo, lower = up ? u_lo : u_hi;
        if (rising ? upper - 1 != c : lower != c) return HW;
        ymin = lo + w.ys;
    }
    double yd = ((double)ymin + 0.5) / 5.0 - 0.5;
    if (yd < 0.0) yd = 0.0; else if (yd > (double)H) yd = (double)H;
    yd = ceil(yd);
    return (int)((long long)q * H + (long long)yd);
}
