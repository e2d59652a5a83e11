// COCO polygons as run-length starts (afigan_amd/ops.py polygons_rle): pycocotools' rleFrPoly and the union of one annotation's polygons,
// restated per crossing instead of per upsampled point, and the decode of starts into byte masks.  include/afigan_hip.h and DESIGN.md
// section 20 state the semantics; tests/poly_f64.py is the plain-loop checker.
//   A crossing of rleFrPoly is a pair of consecutive boundary points whose upsampled columns differ, kept only where the lower of the two
//   columns is c = 5 q + 2 with 0 <= q <= W - 1 (then (c + .5) / 5 - .5 = q exactly in fp64, and for no other c is it an integer in range).
//   The two points of a pair always belong to one edge, so an edge's crossings follow from its two end points alone:
//     x-major edge (dx >= dy): its points have every column between its ends once, so the candidates are the c in [min, max - 1]; the rows of
//       the two points are two evaluations of (int)(ys + s t + .5).
//     y-major edge (dx < dy): the column (int)(xs + s t + .5) is monotonic in t; the t at which it passes c is found by bisection (<= 31
//       steps) and the pair is checked against the reference's own rule (u[p] - 1 for a rising pair, u[p] for a falling one), so that a
//       step of two columns, which rounding allows on an edge of more than 2^22 upsampled rows, still gives the reference's crossing.
//   afi_poly_rle_count_kernel  one block per mask.  Pass 1 sums the candidates of the mask's edges (a thread per edge); pass 2 scans them 256
//                              edges at a time and a thread per (edge, candidate column) writes the key (first key index of its polygon << 32 |
//                              a) -- to LDS while the mask has at most AFI_POLY_RLE_LDS_CAP crossings, else to the mask's slice of the workspace.
//                              A bitonic network with every comparator ascending (so the slots past n need not exist) sorts the keys by
//                              (polygon, a); the key's index minus its polygon's first index is its rank, even ranks count +1 and odd ranks -1
//                              (equal neighbours cancel, which is the odd-multiplicity rule); a mask of several polygons is sorted once more
//                              by a.  A block scan of the signs gives the depth; the last key of a group of equal a is a start iff the depth
//                              is zero on exactly one side of the group.  The starts are compacted into the workspace, their number to nstarts.
//   afi_poly_rle_emit_kernel   one block per mask copies its starts to the caller's offsets.
//   afi_rle_decode_kernel      a wave per (mask, 64 columns, 16 rows): a lane owns a column, enters the starts by one binary search and walks
//                              down its rows; the 64 lanes store 64 neighbouring bytes of a row.
// No atomics, no host synchronisation; results are bit-identical from run to run.
#include "../../include/afigan_hip.h"
#include "afi_select.h"
#include "afi_poly_edge.h"

#define POLY_CAP AFI_POLY_RLE_LDS_CAP
#define DEC_ROWS 16

// the polygon of vertex v: the last p in [p0, p1) with voff[p] <= v (polygons may be empty, so offsets repeat)
__device__ __forceinline__ long long poly_of_vertex(const long long* __restrict__ voff, long long p0, long long p1, long long v) {
    long long lo = p0, hi = p1;
    while (hi - lo > 1) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (voff[mid] <= v) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ PolyEdge poly_edge(const double* __restrict__ xy, const long long* __restrict__ voff, long long p, long long v) {
    const long long vn = v + 1 < voff[p + 1] ? v + 1 : voff[p];
    PolyEdge e;
    e.xs = poly_up(xy[2 * v]);
    e.ys = poly_up(xy[2 * v + 1]);
    e.xe = poly_up(xy[2 * vn]);
    e.ye = poly_up(xy[2 * vn + 1]);
    return e;
}

// Ascending sort of k[0 .. n): the bitonic network whose merges start with a mirrored step, so that every comparator puts the smaller key at the
// lower index and a comparator that reaches past n is a no-op (the missing slots behave as keys above all others).
__device__ __forceinline__ void poly_sort(u64* k, int n) {
    int np = 1;
    while (np < n) np <<= 1;
    const int half = np >> 1;
    for (int size = 2; size <= np; size <<= 1) {
        for (int j = size >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < half; t += blockDim.x) {
                int i, l;
                if (j == (size >> 1)) {
                    const int b = t / j, r = t - b * j;
                    i = b * size + r;
                    l = b * size + size - 1 - r;
                } else {
                    const int b = t / j, r = t - b * j;
                    i = 2 * j * b + r;
                    l = i + j;
                }
                if (l < n) {
                    const u64 a = k[i], c = k[l];
                    if (a > c) { k[i] = c; k[l] = a; }
                }
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(256) void afi_poly_rle_count_kernel(const double* __restrict__ xy, const long long* __restrict__ voff,
                                                                 const long long* __restrict__ poff, const int* __restrict__ hw,
                                                                 const long long* __restrict__ cap_off, long long cap_total,
                                                                 u64* __restrict__ ws_keys, int* __restrict__ ws_starts, int* __restrict__ nstarts) {
    __shared__ u64 s_keys[POLY_CAP];
    __shared__ PolyEdge s_edge[256];
    __shared__ int s_qlo[256], s_inc[256], s_first[256];
    __shared__ int wtot[16];
    __shared__ int s_carry;
    const int m = blockIdx.x, tid = threadIdx.x;
    const long long p0 = poff[m], p1 = poff[m + 1];
    const int H = hw[2 * m], W = hw[2 * m + 1], HW = H * W;
    if (p1 <= p0) {                                     // no polygon: the empty mask
        if (tid == 0) nstarts[m] = 0;
        return;
    }
    const long long v0 = voff[p0], v1 = voff[p1], c0 = cap_off[p0], c1 = cap_off[p1];
    // ---- pass 1: the number of crossings
    long long mine = 0;
    for (long long v = v0 + tid; v < v1; v += 256) {
        const long long p = poly_of_vertex(voff, p0, p1, v);
        int qlo;
        const int nc = poly_edge_cands(poly_edge(xy, voff, p, v), W, &qlo);
        mine += nc;
    }
    int n;
    {
        const long long big = mine < 0x7fffffffll ? mine : 0x7fffffffll;           // (saturated: refused below) the block sum through the int scan, in two halves
        int tl, th;
        rpn_block_scan((int)(big & 0xffff), wtot, &tl);
        rpn_block_scan((int)(big >> 16), wtot, &th);
        const long long tot = ((long long)th << 16) + tl;
        // the caller's capacity must hold them (its bound is sum over edges of dx / 5 + 2): never write past the mask's slice
        if (c0 < 0 || c1 > cap_total || c1 < c0 || tot > c1 - c0 || tot > 0x7fffffffll) {
            if (tid == 0) nstarts[m] = -1;
            return;
        }
        n = (int)tot;
    }
    if (n == 0) {
        if (tid == 0) nstarts[m] = 0;
        return;
    }
    u64* keys = n <= POLY_CAP ? s_keys : ws_keys + c0;  // block-uniform
    int* out = ws_starts + c0;
    // ---- pass 2: the keys
    if (tid == 0) s_carry = 0;
    int base = 0;
    for (long long vb = v0; vb < v1; vb += 256) {       // block-uniform trip count
        const long long v = vb + tid;
        const bool on = v < v1;
        int nc = 0, qlo = 0;
        long long pfirst = 0;
        if (on) {
            const long long p = poly_of_vertex(voff, p0, p1, v);
            const PolyEdge e = poly_edge(xy, voff, p, v);
            nc = poly_edge_cands(e, W, &qlo);
            s_edge[tid] = e;
            pfirst = voff[p];
        }
        s_qlo[tid] = qlo;
        int total;
        const int inc = rpn_block_scan(nc, wtot, &total);
        s_inc[tid] = inc;
        __syncthreads();                                // s_inc, s_carry of the chunk before
        // the first key index of this edge's polygon: the exclusive offset of the polygon's first edge, which lies in this chunk or before it
        int first = 0;
        if (on) {
            const long long j0 = pfirst - vb;
            first = j0 < 0 ? s_carry : base + (j0 == 0 ? 0 : s_inc[j0 - 1]);
        }
        s_first[tid] = first;
        __syncthreads();
        for (int i = tid; i < total; i += 256) {
            int lo = 0, hi = 255;                       // the first edge whose inclusive offset exceeds i
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (s_inc[mid] > i) hi = mid; else lo = mid + 1;
            }
            const int r = i - (lo ? s_inc[lo - 1] : 0);
            const int a = poly_crossing(s_edge[lo], s_qlo[lo] + r, H, HW);
            keys[base + i] = ((u64)(unsigned)s_first[lo] << 32) | (u64)(unsigned)a;
        }
        __syncthreads();
        if (tid == 0) {
            const long long last = (v1 - vb < 256 ? v1 - vb : 256) - 1;
            s_carry = s_first[last];
        }
        base += total;
    }
    __syncthreads();
    // ---- by (polygon, a); then rank -> sign, key = a << 1 | (sign < 0)
    poly_sort(keys, n);
    for (int i = tid; i < n; i += 256) {
        const u64 k = keys[i];
        const unsigned first = (unsigned)(k >> 32), a = (unsigned)k;
        keys[i] = ((u64)a << 1) | (u64)((i - (int)first) & 1);
    }
    __syncthreads();
    if (p1 - p0 > 1) poly_sort(keys, n);
    // ---- depth: key = depth << 32 | a
    int run = 0;
    for (int b = 0; b < n; b += 256) {
        const int i = b + tid;
        u64 k = 0;
        int s = 0;
        if (i < n) {
            k = keys[i];
            s = (k & 1) ? -1 : 1;
        }
        int total;
        const int inc = rpn_block_scan(s, wtot, &total);
        if (i < n) keys[i] = ((u64)(unsigned)(run + inc) << 32) | (k >> 1);
        run += total;
    }
    __syncthreads();
    // ---- starts: the last key of a group of equal a, where the union changes across the group
    int cnt = 0;
    for (int b = 0; b < n; b += 256) {
        const int i = b + tid;
        int f = 0;
        unsigned a = 0;
        if (i < n) {
            const u64 k = keys[i];
            a = (unsigned)k;
            if (a < (unsigned)HW && (i == n - 1 || (unsigned)keys[i + 1] != a)) {
                int g = i;                              // the group's first key
                while (g > 0 && (unsigned)keys[g - 1] == a) --g;
                const bool before = g > 0 && (unsigned)(keys[g - 1] >> 32) != 0u, after = (unsigned)(k >> 32) != 0u;
                f = before != after;
            }
        }
        int total;
        const int inc = rpn_block_scan(f, wtot, &total);
        if (f) out[cnt + inc - 1] = (int)a;
        cnt += total;
    }
    if (tid == 0) nstarts[m] = cnt;
}

__global__ __launch_bounds__(256) void afi_poly_rle_emit_kernel(const long long* __restrict__ poff, const long long* __restrict__ cap_off,
                                                                long long cap_total, const int* __restrict__ ws_starts,
                                                                const long long* __restrict__ start_off, int* __restrict__ starts) {
    const int m = blockIdx.x;
    const long long p0 = poff[m], p1 = poff[m + 1];
    if (p1 <= p0) return;
    const long long c0 = cap_off[p0], c1 = cap_off[p1], o = start_off[m], n = start_off[m + 1] - o;
    if (c0 < 0 || c1 > cap_total || n < 0 || n > c1 - c0) return;      // offsets that are not the scan of this call's nstarts
    for (long long i = threadIdx.x; i < n; i += 256) starts[o + i] = ws_starts[c0 + i];
}

// grid: N * xtiles * ybands blocks of 4 waves; a wave = 64 columns x DEC_ROWS rows
__global__ __launch_bounds__(256) void afi_rle_decode_kernel(const int* __restrict__ starts, const long long* __restrict__ soff, int H, int W,
                                                             int xtiles, int ybands, unsigned char* __restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long b = blockIdx.x;
    const int xt = (int)(b % xtiles);
    b /= xtiles;
    const int yb = (int)(b % ybands);
    const long long m = b / ybands;
    const int x = xt * 64 + lane, y0 = (yb * 4 + wave) * DEC_ROWS;
    if (x >= W || y0 >= H) return;
    const int* s = starts + soff[m];
    const long long n = soff[m + 1] - soff[m];
    const long long j0 = (long long)x * H + y0;
    long long lo = 0, hi = n;                           // the number of starts <= j0
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if ((long long)s[mid] <= j0) lo = mid + 1; else hi = mid;
    }
    const int y1 = y0 + DEC_ROWS < H ? y0 + DEC_ROWS : H;
    unsigned char* o = out + ((long long)m * H + y0) * W + x;
    for (int y = y0; y < y1; ++y) {
        const long long j = (long long)x * H + y;
        while (lo < n && (long long)s[lo] <= j) ++lo;
        *o = (unsigned char)(lo & 1);
        o += W;
    }
}

// ------------------------------------------------------------------------------------------------ entry points
long long afi_poly_rle_ws_bytes(long long cap_total) {
    if (cap_total < 0 || cap_total > 0x7fffffffll) return -1;
    return cap_total * 8 + ((cap_total * 4 + 7) & ~7ll);
}

int afi_poly_rle_count(const double* xy, const long long* vert_off, const long long* poly_off, const int* hw, const long long* cap_off, int N,
                       long long cap_total, void* ws, long long ws_bytes, int* nstarts, void* stream) {
    if (N < 0 || cap_total < 0) return AFI_ERR_BAD_ARG;
    if (N == 0) return AFI_OK;
    if (!xy || !vert_off || !poly_off || !hw || !cap_off || !ws || !nstarts) return AFI_ERR_BAD_ARG;
    const long long need = afi_poly_rle_ws_bytes(cap_total);
    if (need < 0 || ((uintptr_t)xy & 7) || ((uintptr_t)vert_off & 7) || ((uintptr_t)poly_off & 7) || ((uintptr_t)hw & 3) ||
        ((uintptr_t)cap_off & 7) || ((uintptr_t)ws & 7) || ((uintptr_t)nstarts & 3))
        return AFI_ERR_UNSUPPORTED;
    if (ws_bytes < need) return AFI_ERR_BAD_ARG;
    u64* keys = (u64*)ws;
    int* tmp = (int*)(keys + cap_total);
    hipLaunchKernelGGL(afi_poly_rle_count_kernel, dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, xy, vert_off, poly_off, hw, cap_off,
                       cap_total, keys, tmp, nstarts);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}

int afi_poly_rle_emit(const long long* poly_off, const long long* cap_off, int N, long long cap_total, const void* ws, long long ws_bytes,
                      const long long* start_off, int* starts, void* stream) {
    if (N < 0 || cap_total < 0) return AFI_ERR_BAD_ARG;
    if (N == 0) return AFI_OK;
    if (!poly_off || !cap_off || !ws || !start_off || !starts) return AFI_ERR_BAD_ARG;
    const long long need = afi_poly_rle_ws_bytes(cap_total);
    if (need < 0 || ((uintptr_t)poly_off & 7) || ((uintptr_t)cap_off & 7) || ((uintptr_t)ws & 7) || ((uintptr_t)start_off & 7) ||
        ((uintptr_t)starts & 3))
        return AFI_ERR_UNSUPPORTED;
    if (ws_bytes < need) return AFI_ERR_BAD_ARG;
    const int* tmp = (const int*)((const u64*)ws + cap_total);
    hipLaunchKernelGGL(afi_poly_rle_emit_kernel, dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, poly_off, cap_off, cap_total, tmp, start_off,
                       starts);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}

int afi_rle_decode(const int* starts, const long long* start_off, int N, int H, int W, unsigned char* out, void* stream) {
    if (N < 0 || H <= 0 || W <= 0) return AFI_ERR_BAD_ARG;
    if (N == 0) return AFI_OK;
    if (!starts || !start_off || !out) return AFI_ERR_BAD_ARG;
    const long long xtiles = (W + 63) / 64, ybands = (H + 4 * DEC_ROWS - 1) / (4 * DEC_ROWS);
    if ((long long)H * W >= 0x80000000ll || (long long)N * xtiles * ybands > 0x7fffffffll || ((uintptr_t)starts & 3) || ((uintptr_t)start_off & 7))
        return AFI_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(afi_rle_decode_kernel, dim3((unsigned)(N * xtiles * ybands)), dim3(256), 0, (hipStream_t)stream, starts, start_off, H, W,
                       (int)xtiles, (int)ybands, out);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}
