// COCO detection evaluation on the device (afigan_amd/coco_eval.py): the IoU matrices and the greedy matching of pycocotools' COCOeval, whose
// precision / recall accumulation stays on the host.  Work comes in GROUPS, one per (image, category): D detections (sorted by descending score
// and cut by the caller) and G ground truths, given as CSR offsets dt_off / gt_off [ngroups + 1] into the per-detection and per-GT arrays and
// iou_off [ngroups + 1] into the packed matrices (group i: [D][G] row-major at iou_off[i], iou_off[i + 1] - iou_off[i] = D G).
// All arithmetic is fp64 with contraction off, so a numpy restatement gives the same bits (tests/coco_eval_f64.py).
//   afi_coco_box_iou_kernel   a thread per matrix element (grid-stride over the packed matrices); the element's group by a binary search of iou_off.
//   afi_coco_rle_area_kernel  a thread per mask: the sum of the set runs of its ascending run starts.
//   afi_coco_rle_iou_kernel   a thread per pair.  Both masks are zero before lo = max(first starts) and one is zero from hi = min(last ends) on:
//                             lo >= hi (disjoint column ranges, the common pair) is answered from four loads; otherwise each list is entered by
//                             a binary search for lo and the two-pointer merge stops at hi.
//   afi_coco_match_kernel     a wave per group, a lane per (area range, threshold); each lane walks the detections in order.  <false>: G <= 64,
//                             the ignore / crowd / matched flags of the GTs are 64-bit masks in registers and the two walks (non-ignored, then
//                             ignored) are ctz loops.  <true>: any G, the lane's matched flags are bytes of the caller's workspace,
//                             [gt][lane] so that the lanes of a wave touch neighbouring bytes, zeroed by the lane that reads them.
//                             <true> is launched only when the caller's bound max_g on G says that such a group can exist.
//                             The IoU row of a detection is read from global memory by all lanes at the same address (one broadcast load).
// No atomics, no host synchronisation; results are bit-identical from run to run.
#include "../../include/afigan_hip.h"
#include "afi_common.h"

typedef unsigned long long cu64;

// the group of packed element e: the last i with off[i] <= e (groups may be empty, so offsets repeat)
__device__ __forceinline__ int coco_group_of(const long long* __restrict__ off, int ngroups, long long e) {
    int lo = 0, hi = ngroups;                            // invariant: off[lo] <= e < off[hi]
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (off[mid] <= e) lo = mid; else hi = mid;
    }
    return lo;
}

// ------------------------------------------------------------------------------------------------ box IoU
__global__ __launch_bounds__(256) void afi_coco_box_iou_kernel(const double* __restrict__ dt, const double* __restrict__ gt,
                                                               const unsigned char* __restrict__ iscrowd, const long long* __restrict__ dt_off,
                                                               const long long* __restrict__ gt_off, const long long* __restrict__ iou_off,
                                                               int ngroups, long long total, double* __restrict__ iou) {
#pragma clang fp contract(off)
    const long long step = (long long)gridDim.x * 256;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += step) {
        if (e >= iou_off[ngroups]) return;
        const int grp = coco_group_of(iou_off, ngroups, e);
        const long long d0 = dt_off[grp], g0 = gt_off[grp], D = dt_off[grp + 1] - d0, G = gt_off[grp + 1] - g0;
        if (G <= 0) continue;
        const long long loc = e - iou_off[grp], d = loc / G, g = loc - d * G;
        if (d >= D) continue;
        const double* a = dt + 4 * (d0 + d);
        const double* b = gt + 4 * (g0 + g);
        const double dx = a[0], dy = a[1], dw = a[2], dh = a[3], gx = b[0], gy = b[1], gw = b[2], gh = b[3];
        const double w = fmin(dx + dw, gx + gw) - fmax(dx, gx), h = fmin(dy + dh, gy + gh) - fmax(dy, gy);
        double o = 0.0;
        if (w > 0.0 && h > 0.0) {
            const double i = w * h;
            const double u = iscrowd[g0 + g] ? dw * dh : dw * dh + gw * gh - i;
            o = i / u;
        }
        iou[e] = o;
    }
}

// ------------------------------------------------------------------------------------------------ RLE area and IoU
__global__ __launch_bounds__(256) void afi_coco_rle_area_kernel(const int* __restrict__ starts, const long long* __restrict__ soff,
                                                                const int* __restrict__ hw, long long nmask, long long* __restrict__ area) {
    const long long m = (long long)blockIdx.x * 256 + threadIdx.x;
    if (m >= nmask) return;
    const int* s = starts + soff[m];
    const long long n = soff[m + 1] - soff[m];
    long long a = 0;
    for (long long i = 0; i + 1 < n; i += 2) a += (long long)s[i + 1] - (long long)s[i];
    if (n & 1) a += (long long)hw[m] - (long long)s[n - 1];
    area[m] = a;
}

// the number of starts below v
__device__ __forceinline__ long long coco_lower_bound(const int* __restrict__ s, long long n, long long v) {
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if ((long long)s[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void afi_coco_rle_iou_kernel(const int* __restrict__ dt_starts, const long long* __restrict__ dt_soff,
                                                               const int* __restrict__ dt_hw, const long long* __restrict__ dt_area,
                                                               const int* __restrict__ gt_starts, const long long* __restrict__ gt_soff,
                                                               const int* __restrict__ gt_hw, const long long* __restrict__ gt_area,
                                                               const unsigned char* __restrict__ iscrowd, const long long* __restrict__ dt_off,
                                                               const long long* __restrict__ gt_off, const long long* __restrict__ iou_off,
                                                               int ngroups, long long total, long long* __restrict__ inter,
                                                               double* __restrict__ iou) {
#pragma clang fp contract(off)
    const long long step = (long long)gridDim.x * 256;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += step) {
        if (e >= iou_off[ngroups]) return;
        const int grp = coco_group_of(iou_off, ngroups, e);
        const long long d0 = dt_off[grp], g0 = gt_off[grp], D = dt_off[grp + 1] - d0, G = gt_off[grp + 1] - g0;
        if (G <= 0) continue;
        const long long loc = e - iou_off[grp], dl = loc / G, gl = loc - dl * G;
        if (dl >= D) continue;
        const long long d = d0 + dl, g = g0 + gl;
        const long long N = dt_hw[d];
        long long in = -1;
        double o = -1.0;                                 // masks of different sizes: -1, as pycocotools' rleIou
        if (N == (long long)gt_hw[g]) {
            const int* a = dt_starts + dt_soff[d];
            const int* b = gt_starts + gt_soff[g];
            const long long na = dt_soff[d + 1] - dt_soff[d], nb = gt_soff[g + 1] - gt_soff[g];
            in = 0;
            if (na > 0 && nb > 0) {
                const long long a0 = a[0], b0 = b[0], ae = (na & 1) ? N : (long long)a[na - 1], be = (nb & 1) ? N : (long long)b[nb - 1];
                const long long lo = a0 > b0 ? a0 : b0, hi = ae < be ? ae : be;
                if (lo < hi) {
                    long long ia = coco_lower_bound(a, na, lo), ib = coco_lower_bound(b, nb, lo), pos = lo;
                    unsigned va = (unsigned)ia & 1u, vb = (unsigned)ib & 1u;
                    while (pos < hi) {
                        const long long pa = ia < na ? (long long)a[ia] : N, pb = ib < nb ? (long long)b[ib] : N;
                        long long p = pa < pb ? pa : pb;
                        if (p > hi) p = hi;
                        if (va & vb) in += p - pos;
                        pos = p;
                        if (p >= hi) break;
                        if (pa <= pb) { va ^= 1u; ++ia; } else { vb ^= 1u; ++ib; }
                    }
                }
            }
            const long long u = iscrowd[g] ? dt_area[d] : dt_area[d] + gt_area[g] - in;
            o = u == 0 ? 0.0 : (double)in / (double)u;
        }
        if (inter) inter[e] = in;
        iou[e] = o;
    }
}

// ------------------------------------------------------------------------------------------------ greedy matching
// One wave per group.  dt_match / dt_ignore [A][T][total_d], gt_ignore [A][total_g]; ws [total_g][A T] bytes (<true> only).
template <bool BIG>
__global__ __launch_bounds__(64) void afi_coco_match_kernel(const double* __restrict__ iou, const long long* __restrict__ dt_off,
                                                            const long long* __restrict__ gt_off, const long long* __restrict__ iou_off,
                                                            const double* __restrict__ dt_area, const double* __restrict__ gt_area,
                                                            const unsigned char* __restrict__ iscrowd, long long total_d, long long total_g,
                                                            const double* __restrict__ area_rng, int A, const double* __restrict__ iou_thr, int T,
                                                            int max_g, int* __restrict__ dt_match, unsigned char* __restrict__ dt_ignore,
                                                            unsigned char* __restrict__ gt_ignore, unsigned char* __restrict__ ws) {
#pragma clang fp contract(off)
    const int grp = blockIdx.x, lane = threadIdx.x, AT = A * T;
    const long long d0 = dt_off[grp], g0 = gt_off[grp];
    const long long D = dt_off[grp + 1] - d0, G64 = gt_off[grp + 1] - g0;
    if ((G64 > 64) != BIG || G64 > max_g) return;       // block-uniform: the other instantiation's group (or one beyond the caller's bound)
    const int G = (int)G64;                             // A G < 2^31: checked by the entry point on max_g
    const double* M = iou + iou_off[grp];
    for (int i = lane; i < A * G; i += 64) {            // gt_ignore [a][g]
        const int a = i / G, g = i - a * G;
        const double ar = gt_area[g0 + g];
        gt_ignore[(long long)a * total_g + g0 + g] = (iscrowd[g0 + g] || ar < area_rng[2 * a] || ar > area_rng[2 * a + 1]) ? 1 : 0;
    }
    for (int at = lane; at < AT; at += 64) {
        const int a = at / T, t = at - a * T;
        const double lo = area_rng[2 * a], hi = area_rng[2 * a + 1], thr = fmin(iou_thr[t], 1.0 - 1e-10);
        int* om = dt_match + ((long long)at * total_d + d0);
        unsigned char* oi = dt_ignore + ((long long)at * total_d + d0);
        if (!BIG) {
            cu64 ign = 0, crowd = 0, matched = 0;
            for (int g = 0; g < G; ++g) {
                const double ar = gt_area[g0 + g];
                const bool c = iscrowd[g0 + g] != 0;
                if (c) crowd |= 1ull << g;
                if (c || ar < lo || ar > hi) ign |= 1ull << g;
            }
            const cu64 all = G == 64 ? ~0ull : (1ull << G) - 1ull;
            for (long long d = 0; d < D; ++d) {
                const double* row = M + d * G;
                double best = thr;
                int m = -1;
                for (cu64 q = all & ~ign & ~matched; q; q &= q - 1ull) {
                    const int g = __builtin_ctzll(q);
                    const double v = row[g];
                    if (v < best) continue;
                    best = v;
                    m = g;
                }
                if (m < 0)
                    for (cu64 q = ign & (~matched | crowd); q; q &= q - 1ull) {
                        const int g = __builtin_ctzll(q);
                        const double v = row[g];
                        if (v < best) continue;
                        best = v;
                        m = g;
                    }
                unsigned char ig;
                if (m >= 0) {
                    matched |= 1ull << m;
                    ig = (unsigned char)((ign >> m) & 1ull);
                } else {
                    const double ar = dt_area[d0 + d];
                    ig = (ar < lo || ar > hi) ? 1 : 0;
                }
                om[d] = m;
                oi[d] = ig;
            }
        } else {
            unsigned char* mt = ws + g0 * AT + at;      // this lane's matched flag of GT g: mt[g AT]
            for (int g = 0; g < G; ++g) mt[(long long)g * AT] = 0;
            for (long long d = 0; d < D; ++d) {
                const double* row = M + d * G;
                double best = thr;
                int m = -1;
                bool mig = false;
                for (int pass = 0; pass < 2 && m < 0; ++pass)
                    for (int g = 0; g < G; ++g) {
                        const double ar = gt_area[g0 + g];
                        const bool c = iscrowd[g0 + g] != 0, ig = c || ar < lo || ar > hi;
                        if (ig != (pass == 1)) continue;
                        if (mt[(long long)g * AT] && !c) continue;
                        const double v = row[g];
                        if (v < best) continue;
                        best = v;
                        m = g;
                        mig = ig;
                    }
                unsigned char ig;
                if (m >= 0) {
                    mt[(long long)m * AT] = 1;
                    ig = mig ? 1 : 0;
                } else {
                    const double ar = dt_area[d0 + d];
                    ig = (ar < lo || ar > hi) ? 1 : 0;
                }
                om[d] = m;
                oi[d] = ig;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ entry points
static unsigned coco_grid(long long total) {
    const long long b = (total + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > 8192 ? 8192 : b));
}

int afi_coco_box_iou(const double* dt, const double* gt, const unsigned char* iscrowd, const long long* dt_off, const long long* gt_off,
                     const long long* iou_off, int ngroups, long long total, double* iou, void* stream) {
    if (ngroups < 0 || total < 0) return AFI_ERR_BAD_ARG;
    if (ngroups == 0 || total == 0) return AFI_OK;
    if (!dt || !gt || !iscrowd || !dt_off || !gt_off || !iou_off || !iou) return AFI_ERR_BAD_ARG;
    if (((uintptr_t)dt & 7) || ((uintptr_t)gt & 7) || ((uintptr_t)dt_off & 7) || ((uintptr_t)gt_off & 7) || ((uintptr_t)iou_off & 7) ||
        ((uintptr_t)iou & 7))
        return AFI_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(afi_coco_box_iou_kernel, dim3(coco_grid(total)), dim3(256), 0, (hipStream_t)stream, dt, gt, iscrowd, dt_off, gt_off, iou_off,
                       ngroups, total, iou);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}

int afi_coco_rle_area(const int* starts, const long long* start_off, const int* hw, long long nmask, long long* area, void* stream) {
    if (nmask < 0) return AFI_ERR_BAD_ARG;
    if (nmask == 0) return AFI_OK;
    if (!starts || !start_off || !hw || !area) return AFI_ERR_BAD_ARG;
    if (((uintptr_t)starts & 3) || ((uintptr_t)start_off & 7) || ((uintptr_t)hw & 3) || ((uintptr_t)area & 7) || (nmask + 255) / 256 > 0x7fffffffll)
        return AFI_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(afi_coco_rle_area_kernel, dim3((unsigned)((nmask + 255) / 256)), dim3(256), 0, (hipStream_t)stream, starts, start_off, hw,
                       nmask, area);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}

int afi_coco_rle_iou(const int* dt_starts, const long long* dt_start_off, const int* dt_hw, const long long* dt_area, const int* gt_starts,
                     const long long* gt_start_off, const int* gt_hw, const long long* gt_area, const unsigned char* iscrowd,
                     const long long* dt_off, const long long* gt_off, const long long* iou_off, int ngroups, long long total, long long* inter,
                     double* iou, void* stream) {
    if (ngroups < 0 || total < 0) return AFI_ERR_BAD_ARG;
    if (ngroups == 0 || total == 0) return AFI_OK;
    if (!dt_starts || !dt_start_off || !dt_hw || !dt_area || !gt_starts || !gt_start_off || !gt_hw || !gt_area || !iscrowd || !dt_off || !gt_off ||
        !iou_off || !iou)
        return AFI_ERR_BAD_ARG;
    if (((uintptr_t)dt_starts & 3) || ((uintptr_t)gt_starts & 3) || ((uintptr_t)dt_hw & 3) || ((uintptr_t)gt_hw & 3) ||
        ((uintptr_t)dt_start_off & 7) || ((uintptr_t)gt_start_off & 7) || ((uintptr_t)dt_area & 7) || ((uintptr_t)gt_area & 7) ||
        ((uintptr_t)dt_off & 7) || ((uintptr_t)gt_off & 7) || ((uintptr_t)iou_off & 7) || ((uintptr_t)inter & 7) || ((uintptr_t)iou & 7))
        return AFI_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(afi_coco_rle_iou_kernel, dim3(coco_grid(total)), dim3(256), 0, (hipStream_t)stream, dt_starts, dt_start_off, dt_hw, dt_area,
                       gt_starts, gt_start_off, gt_hw, gt_area, iscrowd, dt_off, gt_off, iou_off, ngroups, total, inter, iou);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}

long long afi_coco_match_ws_bytes(long long total_g, int A, int T) {
    if (total_g < 0 || A <= 0 || T <= 0 || (long long)A * T > 4096) return -1;
    return total_g * A * T;
}

int afi_coco_match(const double* iou, const long long* dt_off, const long long* gt_off, const long long* iou_off, int ngroups,
                   const double* dt_area, const double* gt_area, const unsigned char* iscrowd, long long total_d, long long total_g,
                   const double* area_rng, int A, const double* iou_thr, int T, int max_g, int* dt_match, unsigned char* dt_ignore,
                   unsigned char* gt_ignore, void* ws, long long ws_bytes, void* stream) {
    if (ngroups < 0 || total_d < 0 || total_g < 0 || A <= 0 || T <= 0 || max_g < 0) return AFI_ERR_BAD_ARG;
    if (ngroups == 0) return AFI_OK;
    if (!dt_off || !gt_off || !iou_off || !area_rng || !iou_thr) return AFI_ERR_BAD_ARG;
    if ((total_d > 0 && (!dt_area || !dt_match || !dt_ignore)) || (total_g > 0 && (!gt_area || !iscrowd || !gt_ignore || !ws)) ||
        (total_d > 0 && total_g > 0 && !iou))
        return AFI_ERR_BAD_ARG;
    const long long need = afi_coco_match_ws_bytes(total_g, A, T);
    if (need < 0 || (long long)A * max_g > 0x7fffffffll) return AFI_ERR_UNSUPPORTED;
    if (ws_bytes < need) return AFI_ERR_BAD_ARG;
    if (((uintptr_t)iou & 7) || ((uintptr_t)dt_off & 7) || ((uintptr_t)gt_off & 7) || ((uintptr_t)iou_off & 7) || ((uintptr_t)dt_area & 7) ||
        ((uintptr_t)gt_area & 7) || ((uintptr_t)area_rng & 7) || ((uintptr_t)iou_thr & 7) || ((uintptr_t)dt_match & 3))
        return AFI_ERR_UNSUPPORTED;
    // a launch covers all groups and returns at once from those of the other instantiation; the second is made only if max_g admits such a group
    hipLaunchKernelGGL(afi_coco_match_kernel<false>, dim3((unsigned)ngroups), dim3(64), 0, (hipStream_t)stream, iou, dt_off, gt_off, iou_off,
                       dt_area, gt_area, iscrowd, total_d, total_g, area_rng, A, iou_thr, T, max_g, dt_match, dt_ignore, gt_ignore, (unsigned char*)ws);
    if (max_g > 64)
        hipLaunchKernelGGL(afi_coco_match_kernel<true>, dim3((unsigned)ngroups), dim3(64), 0, (hipStream_t)stream, iou, dt_off, gt_off, iou_off,
                           dt_area, gt_area, iscrowd, total_d, total_g, area_rng, A, iou_thr, T, max_g, dt_match, dt_ignore, gt_ignore,
                           (unsigned char*)ws);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}
