// The training side of the mask branch of StandardROIHeads (afigan_amd/roi_heads.py: _ROIMaskLossFn): detectron2 v0.1.1's mask_rcnn_loss on
// the foreground prefix of the box branch's training list -- PolygonMasks.crop_and_resize / rasterize_polygons_within_box for the targets,
// binary cross-entropy with logits (mean) on the row's own class, and the backward of the class-selected predictor.  include/afigan_hip.h and
// DESIGN.md section 23 state the semantics; tests/mask_loss_f64.py is the plain-loop checker.
//   afi_mask_targets    one block per row of the prefix [N][Bf].  The row's matched instance is found as afi_roi_gather_samples finds it; every
//                       vertex of its polygons is moved into the box's M x M frame (one fp64 subtraction, one fp64 product) and upsampled by
//                       afi_poly_edge.h's poly_up, so the edges, candidates and crossings are poly_rle.hip's own text.  On a canvas of at most
//                       28 x 28 no sort is needed: per polygon a table of M M + 1 positions in LDS takes one integer XOR per crossing (a thread
//                       per edge walks its <= M candidates), a block scan of the table is the parity of the starts at or before each
//                       position -- the polygon's mask in column-major order -- and the polygons are ORed into the row's mask.  A row whose
//                       transformed coordinates are not all finite with |5 c + .5| < 2^30 is zero (the comparison is made on the double, so no
//                       out-of-range conversion to int happens).  Every byte of the output is written; counts_fg is written too.
//   afi_mask_loss       afi_roi_mask_probs' shape (lanes across channels, 16-byte loads, class and weight row wave-uniform) and its logit, then
//                       the stable BCE term and d loss / d logit in fp64 from the fp32 logit, both from one pass over h.  The terms: a lane
//                       its pixels in order, a fixed butterfly, the waves of a block in order, the blocks' partials by a second launch in a
//                       fixed order.  Mtot = M M sum(counts_fg) is formed on the device.
//   afi_mask_pred_bwd   dh = dz w[class] (h > 0) over the whole tensor (zeros on padding rows), and per (row, pixel part) the fp32 sums of
//                       dz h[k] and dz in pixel order; a second launch adds the partials of each class in row order (fp64, rounded once) into
//                       dW and db, zero for a class without a row.
// No float atomics, nothing synchronises with the host, every output is bit-identical from run to run.
#include "../../include/afigan_hip.h"
#include "afi_common.h"
#include "afi_select.h"
#include "afi_poly_edge.h"

#define MASKL_MAX_S 14
#define MASKL_MAX_M (2 * MASKL_MAX_S)
#define MASKL_GPW 8                 // afi_roi_mask_probs' pixel groups per wave
#define MASKL_PARTS 8               // pixel parts of a row in afi_mask_pred_bwd
#define MASKL_MAX_C 1024

__device__ __forceinline__ int maskl_clamp(int c, int hi) { return c < 0 ? 0 : (c > hi ? hi : c); }

// ------------------------------------------------------------------------------------------------ targets
// (c - o) r: one rounded subtraction, one rounded product
__device__ __forceinline__ double maskl_tx(double c, double o, double r) {
#pragma clang fp contract(off)
    const double d = c - o;
    return d * r;
}

// M / max(side, 0.1) as numpy forms it: the float32 quotient when max() returns the float32 side (a NaN side too), the float64 one otherwise
__device__ __forceinline__ double maskl_ratio(float side, int M) {
#pragma clang fp contract(off)
    if (!((double)side < 0.1)) return (double)((float)M / side);
    return (double)M / 0.1;
}

__device__ __forceinline__ bool maskl_bad(double c) {
#pragma clang fp contract(off)
    const double m = 5.0 * c;
    return !(fabs(m + 0.5) < 1073741824.0);             // NaN and infinities fail the comparison
}

__global__ __launch_bounds__(256) void afi_mask_targets_kernel(const double* __restrict__ xy, const long long* __restrict__ voff,
                                                               const long long* __restrict__ poff, long long P, long long V,
                                                               const float* __restrict__ boxes, const int* __restrict__ sidx, int B,
                                                               const int* __restrict__ midx, int R, const int* __restrict__ counts_g, int Gmax,
                                                               const int* __restrict__ n_pos, int Bf, int M,
                                                               unsigned char* __restrict__ targets, int* __restrict__ counts_fg) {
#pragma clang fp contract(off)
    __shared__ int s_par[MASKL_MAX_M * MASKL_MAX_M + 1];
    __shared__ unsigned char s_mask[MASKL_MAX_M * MASKL_MAX_M];
    __shared__ int wtot[16];
    __shared__ int s_flag;
    const int row = blockIdx.x, n = row / Bf, j = row - n * Bf, tid = threadIdx.x, MM = M * M;
    const int np = maskl_clamp(n_pos[n], Bf);
    if (j == 0 && tid == 0) counts_fg[n] = np;
    for (int i = tid; i < MM; i += 256) s_mask[i] = 0;
    if (tid == 0) s_flag = 0;
    // everything up to the barrier is block-uniform
    bool live = j < np;
    long long p0 = 0, p1 = 0, v0 = 0, v1 = 0;
    if (live) {
        const int G = maskl_clamp(counts_g[n], Gmax);
        const int i = sidx[(long long)n * B + j];
        live = G > 0 && i >= 0 && i < R;
        if (live) {
            int g = midx[(long long)n * R + i];
            g = g < 0 ? 0 : (g >= G ? G - 1 : g);
            const long long ann = (long long)n * Gmax + g;
            p0 = poff[ann];
            p1 = poff[ann + 1];
            live = p0 >= 0 && p1 <= P && p0 < p1;      // no polygon: the empty mask
        }
        if (live) {
            v0 = voff[p0];
            v1 = voff[p1];
            live = v0 >= 0 && v1 <= V && v0 < v1;
        }
    }
    const float* b = boxes + ((long long)n * B + j) * 4;
    const float bx0 = b[0], by0 = b[1];
    const float bw = b[2] - bx0, bh = b[3] - by0;
    const double ox = (double)bx0, oy = (double)by0, rw = maskl_ratio(bw, M), rh = maskl_ratio(bh, M);
    __syncthreads();
    if (live) {
        bool bad = false;
        for (long long v = v0 + tid; v < v1; v += 256)
            bad = bad || maskl_bad(maskl_tx(xy[2 * v], ox, rw)) || maskl_bad(maskl_tx(xy[2 * v + 1], oy, rh));
        if (bad) s_flag = 1;
    }
    __syncthreads();
    if (live && s_flag == 0) {
        for (long long p = p0; p < p1; ++p) {
            const long long a = voff[p], e1 = voff[p + 1];
            if (a < v0 || e1 > v1 || e1 <= a) continue;             // (block-uniform) an empty polygon, or offsets that do not nest
            for (int i = tid; i <= MM; i += 256) s_par[i] = 0;
            __syncthreads();
            for (long long v = a + tid; v < e1; v += 256) {
                const long long vn = v + 1 < e1 ? v + 1 : a;
                PolyEdge e;
                e.xs = poly_up(maskl_tx(xy[2 * v], ox, rw));
                e.ys = poly_up(maskl_tx(xy[2 * v + 1], oy, rh));
                e.xe = poly_up(maskl_tx(xy[2 * vn], ox, rw));
                e.ye = poly_up(maskl_tx(xy[2 * vn + 1], oy, rh));
                int qlo;
                const int nc = poly_edge_cands(e, M, &qlo);        // <= M: the candidates are clipped to the canvas
                for (int r = 0; r < nc; ++r) {
                    const int c = poly_crossing(e, qlo + r, M, MM);
                    if (c >= 0 && c <= MM) atomicXor(&s_par[c], 1);
                }
            }
            __syncthreads();
            int run = 0;
            for (int i0 = 0; i0 < MM; i0 += 256) {                  // position i = x M + y: the parity of the crossings at or before it
                const int i = i0 + tid;
                int total;
                const int inc = rpn_block_scan(i < MM ? s_par[i] : 0, wtot, &total);
                if (i < MM && ((run + inc) & 1)) {
                    const int x = i / M, y = i - x * M;
                    s_mask[y * M + x] = 1;
                }
                run += total;
            }
            __syncthreads();
        }
    }
    __syncthreads();
    unsigned char* o = targets + (long long)row * MM;
    for (int i = tid; i < MM; i += 256) o[i] = s_mask[i];
}

int afi_mask_targets(const double* xy, const long long* vert_off, const long long* poly_off, long long num_poly, long long num_vert,
                     const float* boxes, const int* sampled_idx, int N, int batch_per_image, const int* matched_idx, int ld_matched,
                     const int* counts_g, int Gmax, const int* n_pos, int Bf, int M, unsigned char* targets, int* counts_fg, void* stream) {
    if (!xy || !vert_off || !poly_off || !boxes || !sampled_idx || !matched_idx || !counts_g || !n_pos || !targets || !counts_fg || N <= 0 ||
        N > 65535 || batch_per_image <= 0 || ld_matched <= 0 || Gmax <= 0 || Bf <= 0 || Bf > batch_per_image || M <= 0 || num_poly < 0 ||
        num_vert < 0)
        return AFI_ERR_BAD_ARG;
    if (M > MASKL_MAX_M || batch_per_image > 4096 || ((uintptr_t)xy & 7) || ((uintptr_t)vert_off & 7) || ((uintptr_t)poly_off & 7) ||
        ((uintptr_t)boxes & 3))
        return AFI_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(afi_mask_targets_kernel, dim3((unsigned)(N * Bf)), dim3(256), 0, (hipStream_t)stream, xy, vert_off, poly_off, num_poly,
                       num_vert, boxes, sampled_idx, batch_per_image, matched_idx, ld_matched, counts_g, Gmax, n_pos, Bf, M, targets, counts_fg);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}

// ------------------------------------------------------------------------------------------------ loss and d loss / d logit
// Mtot = M M sum of counts (each clamped to 0 .. D), the same value in every lane: integers, so the order does not matter.
__device__ __forceinline__ long long maskl_mtot(const int* __restrict__ counts, int N, int D, int S) {
    long long s = 0;
    for (int n = threadIdx.x & 63; n < N; n += 64) s += maskl_clamp(counts[n], D);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    return s * 4 * S * S;
}

__device__ __forceinline__ int maskl_row_class(const int* __restrict__ classes, int ld, int n, int d, int Km) {
    return Km == 1 ? 0 : classes[(long long)n * ld + d];
}

// LW, G, gpr, wpr: afi_roi_mask_probs_kernel's.  partial[b]: block b's sum of the terms.
__global__ __launch_bounds__(256) void afi_mask_loss_kernel(const float4* __restrict__ h, const float4* __restrict__ w,
                                                            const float* __restrict__ bias, const int* __restrict__ classes, int ldc,
                                                            const int* __restrict__ counts, const unsigned char* __restrict__ targets, int N,
                                                            int D, int C4, int S, int Km, int LW, int G, int gpr, int wpr,
                                                            float* __restrict__ dz, double* __restrict__ partial) {
    __shared__ double wsum[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long wv = (long long)blockIdx.x * 4 + wave, total = (long long)N * D * wpr;
    const long long mtot = maskl_mtot(counts, N, D, S);
    double tacc = 0.0;
    if (wv < total) {
        const long long row = wv / wpr;
        const int part = (int)(wv - row * wpr), n = (int)(row / D), d = (int)(row - (long long)n * D);
        const int P4 = 4 * S * S, M = 2 * S;
        const int sub = lane / LW, c0 = lane - sub * LW;
        const int cls = __builtin_amdgcn_readfirstlane(maskl_row_class(classes, ldc, n, d, Km));
        const bool live = d < maskl_clamp(counts[n], D) && cls >= 0 && cls < Km;       // wave-uniform
        const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
        const float4* wr = w + (long long)(live ? cls : 0) * C4;
        const float bz = live ? bias[cls] : 0.f;
        const float4 wreg = (live && c0 < C4) ? wr[c0] : zero;
        for (int k = 0; k < MASKL_GPW; ++k) {
            const int g = part * MASKL_GPW + k;
            if (g >= gpr) break;
            const int q = g * G + sub;
            const bool on = sub < G && q < P4;
            float acc = 0.f;
            if (live && on) {
                const float4* hp = h + (row * P4 + q) * C4;
                if (C4 <= 64) {
                    if (c0 < C4) {
                        const float4 f = hp[c0];
                        acc = fmaf(wreg.w, f.w, fmaf(wreg.z, f.z, fmaf(wreg.y, f.y, fmaf(wreg.x, f.x, acc))));
                    }
                } else {
                    for (int c = c0; c < C4; c += 64) {
                        const float4 f = hp[c], u = wr[c];
                        acc = fmaf(u.w, f.w, fmaf(u.z, f.z, fmaf(u.y, f.y, fmaf(u.x, f.x, acc))));
                    }
                }
            }
            for (int o = LW >> 1; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
            if (on && c0 == 0) {
                float gz = 0.f;
                if (live) {
                    const int pix = q >> 2, ph = q & 3, y = pix / S, x = pix - y * S;
                    const double z = (double)(acc + bz);
                    const double t = targets[row * P4 + (long long)(2 * y + (ph >> 1)) * M + 2 * x + (ph & 1)] ? 1.0 : 0.0;
                    tacc += (fmax(z, 0.0) - z * t) + log1p(exp(-fabs(z)));
                    gz = (float)((1.0 / (1.0 + exp(-z)) - t) / (double)mtot);
                }
                dz[row * P4 + q] = gz;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) tacc += __shfl_xor(tacc, o, 64);
    if (lane == 0) wsum[wave] = tacc;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

__global__ __launch_bounds__(256) void afi_mask_loss_final_kernel(const double* __restrict__ partial, long long nblocks,
                                                                  const int* __restrict__ counts, int N, int D, int S, float* __restrict__ loss) {
    __shared__ double s[256];
    const long long mtot = maskl_mtot(counts, N, D, S);
    double a = 0.0;
    for (long long i = threadIdx.x; i < nblocks; i += 256) a += partial[i];
    s[threadIdx.x] = a;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = mtot > 0 ? (float)(s[0] / (double)mtot) : 0.f;
}

struct MasklShape { int C4, P4, LW, G, gpr, wpr; long long blocks; };

static bool maskl_shape(int N, int D, int C, int S, MasklShape* q) {
    if (N <= 0 || N > 65535 || D <= 0 || C <= 0 || (C & 3) || S <= 0 || S > MASKL_MAX_S) return false;
    q->C4 = C / 4;
    q->P4 = 4 * S * S;
    q->LW = 64;
    if (q->C4 < 64) { q->LW = 1; while (q->LW < q->C4) q->LW <<= 1; }
    q->G = 64 / q->LW;
    q->gpr = (q->P4 + q->G - 1) / q->G;
    q->wpr = (q->gpr + MASKL_GPW - 1) / MASKL_GPW;
    q->blocks = ((long long)N * D * q->wpr + 3) / 4;
    return q->blocks <= 0x7fffffffll;
}

long long afi_mask_loss_ws_floats(int N, int D, int C, int S) {
    MasklShape q;
    return maskl_shape(N, D, C, S, &q) ? 2 * q.blocks : -1;
}

int afi_mask_loss(const float* h, const float* w, const float* bias, const int* classes, int ld_classes, const int* counts_fg,
                  const unsigned char* targets, int N, int D, int C, int S, int Km, float* loss, float* dz, float* ws, long long ws_floats,
                  void* stream) {
    if (!h || !w || !bias || !classes || !counts_fg || !targets || !loss || !dz || N <= 0 || N > 65535 || D <= 0 || C <= 0 || S <= 0 || Km <= 0 ||
        ld_classes < D)
        return AFI_ERR_BAD_ARG;
    MasklShape q;
    if (!maskl_shape(N, D, C, S, &q) || ((uintptr_t)h & 15) || ((uintptr_t)w & 15) || ((uintptr_t)dz & 3) || ((uintptr_t)bias & 3))
        return AFI_ERR_UNSUPPORTED;
    if (!ws || ws_floats < 2 * q.blocks || ((uintptr_t)ws & 7)) return AFI_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(afi_mask_loss_kernel, dim3((unsigned)q.blocks), dim3(256), 0, st, (const float4*)h, (const float4*)w, bias, classes,
                       ld_classes, counts_fg, targets, N, D, q.C4, S, Km, q.LW, q.G, q.gpr, q.wpr, dz, (double*)ws);
    hipLaunchKernelGGL(afi_mask_loss_final_kernel, dim3(1), dim3(256), 0, st, (const double*)ws, q.blocks, counts_fg, N, D, S, loss);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}

// ------------------------------------------------------------------------------------------------ backward of the class-selected predictor
// grid (MASKL_PARTS, R).  LW lanes per pixel (a power of two >= C4), nsub = 256 / LW pixels side by side; part `part` owns pixels
// [part ppp, (part + 1) ppp).  partial [R][MASKL_PARTS][C + 4]: the sums of dz h[k], then of dz, then three zeros.
__global__ __launch_bounds__(256) void afi_mask_pred_bwd_kernel(const float4* __restrict__ h, const float* __restrict__ dz,
                                                                const float4* __restrict__ w, const int* __restrict__ classes, int ldc,
                                                                const int* __restrict__ counts, int D, int C4, int P4, int Km, int LW, int ppp,
                                                                float4* __restrict__ dh, float4* __restrict__ partial) {
    __shared__ float4 s_acc[256];
    __shared__ float s_z[256];
    const int tid = threadIdx.x, part = blockIdx.x, nsub = 256 / LW, sub = tid / LW, c0 = tid - sub * LW;
    const long long row = blockIdx.y;
    const int n = (int)(row / D), d = (int)(row - (long long)n * D);
    const int cls = maskl_row_class(classes, ldc, n, d, Km);
    const bool live = d < maskl_clamp(counts[n], D) && cls >= 0 && cls < Km;           // block-uniform
    const int qa = part * ppp, qb = qa + ppp < P4 ? qa + ppp : P4;
    if (!live) {                                        // block-uniform: zeros, and its partials are never read
        if (c0 < C4)
            for (int q = qa + sub; q < qb; q += nsub) dh[(row * P4 + q) * C4 + c0] = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    float wx = 0.f, wy = 0.f, wz = 0.f, ww = 0.f;
    float ax = 0.f, ay = 0.f, az = 0.f, aw = 0.f, accz = 0.f;
    if (c0 < C4) {
        const float4 wr = w[(long long)cls * C4 + c0];
        wx = wr.x; wy = wr.y; wz = wr.z; ww = wr.w;
        for (int q = qa + sub; q < qb; q += nsub) {
            const long long i = (row * P4 + q) * C4 + c0;
            const float g = dz[row * P4 + q];
            const float4 f = h[i];
            dh[i] = make_float4(f.x > 0.f ? g * wx : 0.f, f.y > 0.f ? g * wy : 0.f, f.z > 0.f ? g * wz : 0.f, f.w > 0.f ? g * ww : 0.f);
            ax = fmaf(g, f.x, ax); ay = fmaf(g, f.y, ay); az = fmaf(g, f.z, az); aw = fmaf(g, f.w, aw);
            accz += g;
        }
    }
    s_acc[tid] = make_float4(ax, ay, az, aw);
    s_z[tid] = accz;
    __syncthreads();
    if (sub == 0 && c0 < C4) {
        const float4 a0 = s_acc[c0];
        float sx = a0.x, sy = a0.y, sz = a0.z, sw = a0.w, z = s_z[c0];
        for (int s = 1; s < nsub; ++s) {
            const float4 t = s_acc[s * LW + c0];
            sx += t.x; sy += t.y; sz += t.z; sw += t.w;
            z += s_z[s * LW + c0];
        }
        float4* o = partial + (row * MASKL_PARTS + part) * (C4 + 1);
        o[c0] = make_float4(sx, sy, sz, sw);
        if (c0 == 0) o[C4] = make_float4(z, 0.f, 0.f, 0.f);
    }
}

// grid (ceil((C + 1) / 256), Km): thread k of class c adds column k of the partials of the class's rows, in (row, part) order.
__global__ __launch_bounds__(256) void afi_mask_pred_bwd_sum_kernel(const float* __restrict__ partial, const int* __restrict__ classes, int ldc,
                                                                    const int* __restrict__ counts, int N, int D, int C, int Km,
                                                                    float* __restrict__ dW, float* __restrict__ db) {
    const int k = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y;
    if (k > C) return;
    double a = 0.0;
    for (int n = 0; n < N; ++n) {
        const int cnt = maskl_clamp(counts[n], D);
        for (int d = 0; d < cnt; ++d) {
            if (maskl_row_class(classes, ldc, n, d, Km) != c) continue;
            const float* p = partial + ((long long)n * D + d) * MASKL_PARTS * (C + 4) + k;
            for (int s = 0; s < MASKL_PARTS; ++s) a += (double)p[(long long)s * (C + 4)];
        }
    }
    if (k < C) dW[(long long)c * C + k] = (float)a; else db[c] = (float)a;
}

long long afi_mask_pred_bwd_ws_floats(int N, int D, int C) {
    if (N <= 0 || D <= 0 || C <= 0 || (C & 3) || C > MASKL_MAX_C) return -1;
    return (long long)N * D * MASKL_PARTS * (C + 4);
}

int afi_mask_pred_bwd(const float* h, const float* dz, const float* w, const int* classes, int ld_classes, const int* counts_fg, int N, int D,
                      int C, int S, int Km, float* dh, float* dW, float* db, float* ws, long long ws_floats, void* stream) {
    if (!h || !dz || !w || !classes || !counts_fg || !dh || !dW || !db || N <= 0 || N > 65535 || D <= 0 || C <= 0 || S <= 0 || Km <= 0 ||
        ld_classes < D || h == dh)
        return AFI_ERR_BAD_ARG;
    if ((C & 3) || C > MASKL_MAX_C || S > MASKL_MAX_S || Km > 65535 || (long long)N * D > 65535 || ((uintptr_t)h & 15) || ((uintptr_t)w & 15) ||
        ((uintptr_t)dh & 15) || ((uintptr_t)dz & 3))
        return AFI_ERR_UNSUPPORTED;
    const long long need = afi_mask_pred_bwd_ws_floats(N, D, C);
    if (!ws || need < 0 || ws_floats < need || ((uintptr_t)ws & 15)) return AFI_ERR_WORKSPACE;
    const int C4 = C / 4, P4 = 4 * S * S;
    int LW = 1;
    while (LW < C4) LW <<= 1;
    const int ppp = (P4 + MASKL_PARTS - 1) / MASKL_PARTS;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(afi_mask_pred_bwd_kernel, dim3(MASKL_PARTS, (unsigned)(N * D)), dim3(256), 0, st, (const float4*)h, dz, (const float4*)w,
                       classes, ld_classes, counts_fg, D, C4, P4, Km, LW, ppp, (float4*)dh, (float4*)ws);
    hipLaunchKernelGGL(afi_mask_pred_bwd_sum_kernel, dim3((unsigned)((C + 1 + 255) / 256), (unsigned)Km), dim3(256), 0, st, (const float*)ws, classes,
                       ld_classes, counts_fg, N, D, C, Km, dW, db);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}
