// The training side of the box branch of StandardROIHeads (afigan_amd/roi_heads.py: StandardROIHeads.losses): detectron2 v0.1.1's
// ROIHeads.label_and_sample_proposals (add_ground_truth_to_proposals, Matcher without low-quality matches, subsample_labels),
// Box2BoxTransform.get_deltas, FastRCNNOutputs.softmax_cross_entropy_loss / smooth_l1_loss, and the backward of the multi-level ROIAlign.
// The sampling itself is afi_rpn_sample (rpn_loss.hip) on the labels written here.
//   afi_roi_label           one thread per candidate of the padded list [N][P + Gmax] -- the image's counts_p proposals, then (append_gt) its
//                           counts_g ground-truth boxes, the order cat([proposals, gt]) gives; nothing is copied.  The image's boxes and areas in
//                           LDS in tiles of 256; IoU and the running (max, lowest index) from afi_box_match.h.  Label 1 from the threshold up,
//                           0 below, -1 for padding.
//   afi_roi_gather_samples  the padded training list of the sample: boxes, counts, classes (K for background), matched boxes.
//   afi_roi_box_loss        one wave per row: cross-entropy logsumexp - z[gt] in fp64 (the butterfly of roi.hip's softmax), smooth L1 on the
//                           four columns of the row's class in fp32 against the fp64 target rounded once; both sums in fp64 in a fixed order
//                           (a wave its rows in order, a shuffle tree, the waves of a block in order, the blocks' partials in order in a second
//                           launch); the gradient of both losses, the whole dpred tensor written.  Rtot = sum of counts is formed on the device.
//   afi_roi_align_bwd       the owner form: a block owns an 8 x 8 tile of level pixels of one image and level (and 64 float4 of channels), walks
//                           the image's boxes in list order (level and pixel footprint of every box from a pre-pass), forms for each box that
//                           meets the tile the two axis-weight tables of the tile's rows and columns in LDS (fp64 sums of the forward's own 1-D
//                           weights, rounded once) and accumulates in fp32 in (box, ph, pw) order.  Every pixel of every level is written once.
// No float atomics, nothing synchronises with the host, every output is bit-identical from run to run.
#include "../../include/afigan_hip.h"
#include "afi_common.h"
#include "afi_select.h"
#include "afi_box_match.h"

#define ROIL_GT_TILE 256
#define ROIL_MAX_GT 1024
#define ROIL_MAX_K 1024
#define ROIL_MAX_LEVELS 8
#define ROIL_MAX_S 14
#define ROIL_MAX_GRID 4096
#define ROIL_CANON_SIZE 224.0
#define ROIL_CANON_LEVEL 4.0
#define ROIL_TILE 8                 // the owner tile is ROIL_TILE x ROIL_TILE level pixels
#define ROIL_LOSS_BLOCKS 256        // at most this many blocks (and partial sums) in afi_roi_box_loss

// ------------------------------------------------------------------------------------------------ labels
// Candidate i of image n: proposal i below cp, ground-truth box i - cp below cp + cg (append_gt), padding from there on.
__device__ __forceinline__ bool roil_candidate(const float* __restrict__ proposals, const float* __restrict__ gt, int img, int P, int Gmax, int cp,
                                               int cg_app, int i, float4* out) {
    if (i < cp) {
        const float* q = proposals + ((long long)img * P + i) * 4;
        *out = make_float4(q[0], q[1], q[2], q[3]);
        return true;
    }
    if (i - cp < cg_app) {
        const float* q = gt + ((long long)img * Gmax + (i - cp)) * 4;
        *out = make_float4(q[0], q[1], q[2], q[3]);
        return true;
    }
    *out = make_float4(0.f, 0.f, 0.f, 0.f);
    return false;
}

__device__ __forceinline__ int roil_clamp_count(int c, int hi) { return c < 0 ? 0 : (c > hi ? hi : c); }

__global__ __launch_bounds__(256) void afi_roi_label_kernel(const float* __restrict__ proposals, const int* __restrict__ counts_p, int P,
                                                            const float* __restrict__ gt, const int* __restrict__ counts_g, int Gmax,
                                                            int append_gt, float thresh, signed char* __restrict__ labels,
                                                            int* __restrict__ matched_idx) {
    __shared__ float4 sb[ROIL_GT_TILE];
    __shared__ float sa[ROIL_GT_TILE];
    const int img = blockIdx.y, tid = threadIdx.x, R = P + Gmax, i = blockIdx.x * 256 + tid;
    const int cp = roil_clamp_count(counts_p[img], P), G = roil_clamp_count(counts_g[img], Gmax);
    float4 c;
    const bool live = i < R && roil_candidate(proposals, gt, img, P, Gmax, cp, append_gt ? G : 0, i, &c);
    const float carea = afi_box_area(c);
    AfiMatch m{0.f, 0};
    for (int g0 = 0; g0 < G; g0 += ROIL_GT_TILE) {
        const int nt = G - g0 < ROIL_GT_TILE ? G - g0 : ROIL_GT_TILE;
        if (tid < nt) {
            const float* q = gt + ((long long)img * Gmax + g0 + tid) * 4;
            const float4 b = make_float4(q[0], q[1], q[2], q[3]);
            sb[tid] = b;
            sa[tid] = afi_box_area(b);
        }
        __syncthreads();
        if (live)
            for (int j = 0; j < nt; ++j) afi_match_update(m, afi_box_iou(sb[j], sa[j], c, carea), g0 + j);
        __syncthreads();
    }
    if (i >= R) return;
    const long long o = (long long)img * R + i;
    labels[o] = (signed char)(!live ? -1 : (G > 0 ? afi_match_label(m.val, thresh, thresh) : 0));
    matched_idx[o] = live ? m.idx : 0;
}

int afi_roi_label(const float* proposals, const int* counts_p, int N, int P, const float* gt, const int* counts_g, int Gmax, int append_gt,
                  float iou_thresh, signed char* labels, int* matched_idx, void* stream) {
    if (!proposals || !counts_p || !gt || !counts_g || !labels || !matched_idx || N <= 0 || N > 65535 || P <= 0 || Gmax <= 0 ||
        !(iou_thresh == iou_thresh))
        return AFI_ERR_BAD_ARG;
    if (Gmax > ROIL_MAX_GT || (long long)P + Gmax > (1 << 22)) return AFI_ERR_UNSUPPORTED;
    const int R = P + Gmax;
    hipLaunchKernelGGL(afi_roi_label_kernel, dim3((R + 255) / 256, N), dim3(256), 0, (hipStream_t)stream, proposals, counts_p, P, gt, counts_g,
                       Gmax, append_gt ? 1 : 0, iou_thresh, labels, matched_idx);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}

// ------------------------------------------------------------------------------------------------ gather
__global__ __launch_bounds__(256) void afi_roi_gather_kernel(const float* __restrict__ proposals, const int* __restrict__ counts_p, int N, int P,
                                                             const float* __restrict__ gt, const int* __restrict__ gt_classes,
                                                             const int* __restrict__ counts_g, int Gmax, int append_gt,
                                                             const int* __restrict__ matched_idx, const int* __restrict__ sidx,
                                                             const int* __restrict__ n_pos, const int* __restrict__ n_neg, int B, int K,
                                                             float* __restrict__ boxes, int* __restrict__ counts, int* __restrict__ cls,
                                                             float* __restrict__ gboxes) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)N * B) return;
    const int img = (int)(e / B), j = (int)(e - (long long)img * B), R = P + Gmax;
    const int cp = roil_clamp_count(counts_p[img], P), G = roil_clamp_count(counts_g[img], Gmax);
    int np = n_pos[img], nn = n_neg[img];
    np = np < 0 ? 0 : (np > B ? B : np);
    nn = nn < 0 ? 0 : (nn > B - np ? B - np : nn);
    if (j == 0) counts[img] = np + nn;
    float4 b = make_float4(0.f, 0.f, 0.f, 0.f), gb = b;
    int c = -1;
    const int i = j < np + nn ? sidx[e] : -1;
    if (i >= 0 && i < R) {
        roil_candidate(proposals, gt, img, P, Gmax, cp, append_gt ? G : 0, i, &b);
        c = K;
        if (G > 0) {
            int g = matched_idx[(long long)img * R + i];
            g = g < 0 ? 0 : (g >= G ? G - 1 : g);
            const float* q = gt + ((long long)img * Gmax + g) * 4;
            gb = make_float4(q[0], q[1], q[2], q[3]);
            if (j < np) c = gt_classes[(long long)img * Gmax + g];
        }
    }
    *(float4*)(boxes + 4 * e) = b;
    *(float4*)(gboxes + 4 * e) = gb;
    cls[e] = c;
}

int afi_roi_gather_samples(const float* proposals, const int* counts_p, int N, int P, const float* gt, const int* gt_classes, const int* counts_g,
                           int Gmax, int append_gt, const int* matched_idx, const int* sampled_idx, const int* n_pos, const int* n_neg,
                           int batch_per_image, int K, float* boxes, int* counts, int* classes, float* gt_boxes, void* stream) {
    if (!proposals || !counts_p || !gt || !gt_classes || !counts_g || !matched_idx || !sampled_idx || !n_pos || !n_neg || !boxes || !counts ||
        !classes || !gt_boxes || N <= 0 || N > 65535 || P <= 0 || Gmax <= 0 || batch_per_image <= 0 || K <= 0)
        return AFI_ERR_BAD_ARG;
    if (Gmax > ROIL_MAX_GT || K > ROIL_MAX_K || (long long)P + Gmax > (1 << 22) || batch_per_image > 4096 || ((uintptr_t)boxes & 15) ||
        ((uintptr_t)gt_boxes & 15))
        return AFI_ERR_UNSUPPORTED;
    const long long total = (long long)N * batch_per_image;
    hipLaunchKernelGGL(afi_roi_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, proposals, counts_p, N, P,
                       gt, gt_classes, counts_g, Gmax, append_gt ? 1 : 0, matched_idx, sampled_idx, n_pos, n_neg, batch_per_image, K, boxes,
                       counts, classes, gt_boxes);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}

// ------------------------------------------------------------------------------------------------ losses
struct RoiLossArgs {
    int N, B, K, agnostic;
    long long ld;
    float wx, wy, ww, wh, beta;
};

__device__ __forceinline__ double roil_wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double roil_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Rtot = sum of counts (each clamped to 0 .. B), the same value in every lane of every wave: integers, so the order does not matter.
__device__ __forceinline__ long long roil_rtot(const int* __restrict__ counts, int N, int B) {
    long long s = 0;
    for (int n = threadIdx.x & 63; n < N; n += 64) s += roil_clamp_count(counts[n], B);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    return s;
}

// partial[2 b], partial[2 b + 1]: block b's sums of the cross-entropy and of the smooth-L1 terms.
__global__ __launch_bounds__(256) void afi_roi_box_loss_kernel(const RoiLossArgs q, const float* __restrict__ pred, const float* __restrict__ boxes,
                                                               const int* __restrict__ counts, const int* __restrict__ cls,
                                                               const float* __restrict__ gboxes, float* __restrict__ dpred,
                                                               double* __restrict__ partial) {
    __shared__ double wsum[2][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, K = q.K;
    const long long rows = (long long)q.N * q.B, rtot = roil_rtot(counts, q.N, q.B);
    const double inv = rtot > 0 ? 1.0 / (double)rtot : 0.0;
    const float inv32 = (float)inv;
    double acc_cls = 0.0, acc_loc = 0.0;            // acc_cls: the same in every lane; acc_loc: lane c < 4 holds column c's terms
    for (long long row = (long long)blockIdx.x * 4 + wave; row < rows; row += (long long)gridDim.x * 4) {
        const int n = (int)(row / q.B), j = (int)(row - (long long)n * q.B);
        const float* z = pred + row * q.ld;
        float* dz = dpred + row * q.ld;
        const int c_gt = cls[row];
        if (j >= roil_clamp_count(counts[n], q.B) || c_gt < 0 || c_gt > K) {
            for (long long c = lane; c < q.ld; c += 64) dz[c] = 0.f;
            continue;
        }
        double m = -INFINITY;
        for (int c = lane; c <= K; c += 64) m = fmax(m, (double)z[c]);
        m = roil_wave_max(m);
        double s = 0.0;
        for (int c = lane; c <= K; c += 64) s += exp((double)z[c] - m);
        s = roil_wave_sum(s);
        acc_cls += (m + log(s)) - (double)z[c_gt];
        const bool fg = c_gt < K;
        const int base = K + 1 + (q.agnostic ? 0 : 4 * c_gt);
        float gd = 0.f;
        if (fg && lane < 4) {
            // Box2BoxTransform.get_deltas(box, matched box) in fp64 from the fp32 coordinates, rounded once
            const float* a = boxes + 4 * row;
            const float* b = gboxes + 4 * row;
            const double sw = (double)a[2] - (double)a[0], sh = (double)a[3] - (double)a[1];
            const double scx = (double)a[0] + 0.5 * sw, scy = (double)a[1] + 0.5 * sh;
            const double tw = (double)b[2] - (double)b[0], th = (double)b[3] - (double)b[1];
            const double tcx = (double)b[0] + 0.5 * tw, tcy = (double)b[1] + 0.5 * th;
            const float tgt = lane == 0 ? (float)((double)q.wx * (tcx - scx) / sw) : lane == 1 ? (float)((double)q.wy * (tcy - scy) / sh)
                            : lane == 2 ? (float)((double)q.ww * log(tw / sw)) : (float)((double)q.wh * log(th / sh));
            const float d = z[base + lane] - tgt, ad = fabsf(d);
            float term, gr;
            if (q.beta < 1e-5f) {
                term = ad;
                gr = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
            } else if (ad < q.beta) {
                term = 0.5f * d * d / q.beta;
                gr = d / q.beta;
            } else {
                term = ad - 0.5f * q.beta;
                gr = d > 0.f ? 1.f : -1.f;
            }
            acc_loc += (double)term;
            gd = gr * inv32;
        }
        for (long long c0 = 0; c0 < q.ld; c0 += 64) {      // every column of the row is written once, by the lane that owns it
            const long long c = c0 + lane;
            const int rel = (int)(c - base);
            const float gsh = __shfl(gd, rel & 3, 64);      // lanes 0..3 hold the four delta gradients (zero on a background row)
            if (c >= q.ld) continue;
            float v = 0.f;
            if (c <= K) v = (float)((exp((double)z[c] - m) / s - (c == c_gt ? 1.0 : 0.0)) * inv);
            else if (rel >= 0 && rel < 4) v = gsh;
            dz[c] = v;
        }
    }
    acc_loc = roil_wave_sum(acc_loc);
    if (lane == 0) { wsum[0][wave] = acc_cls; wsum[1][wave] = acc_loc; }
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = ((wsum[0][0] + wsum[0][1]) + wsum[0][2]) + wsum[0][3];
        partial[2 * blockIdx.x + 1] = ((wsum[1][0] + wsum[1][1]) + wsum[1][2]) + wsum[1][3];
    }
}

__global__ __launch_bounds__(64) void afi_roi_box_loss_final_kernel(const double* __restrict__ partial, int nblocks, const int* __restrict__ counts,
                                                                    int N, int B, float* __restrict__ loss) {
    const long long rtot = roil_rtot(counts, N, B);
    if (threadIdx.x != 0) return;
    double a = 0.0, b = 0.0;
    for (int i = 0; i < nblocks; ++i) { a += partial[2 * i]; b += partial[2 * i + 1]; }
    loss[0] = rtot > 0 ? (float)(a / (double)rtot) : 0.f;
    loss[1] = rtot > 0 ? (float)(b / (double)rtot) : 0.f;
}

long long afi_roi_box_loss_ws_floats(void) { return 4ll * ROIL_LOSS_BLOCKS; }

int afi_roi_box_loss(const float* pred, long long ld_pred, int N, int batch_per_image, int K, int agnostic, const float* boxes, const int* counts,
                     const int* gt_classes, const float* gt_boxes, float wx, float wy, float ww, float wh, float beta, float* loss, float* dpred,
                     float* ws, long long ws_floats, void* stream) {
    if (!pred || !boxes || !counts || !gt_classes || !gt_boxes || !loss || !dpred || N <= 0 || N > 65535 || batch_per_image <= 0 || K <= 0 ||
        !(beta >= 0.f) || !(wx > 0.f) || !(wy > 0.f) || !(ww > 0.f) || !(wh > 0.f) || pred == dpred)
        return AFI_ERR_BAD_ARG;
    if (K > ROIL_MAX_K || batch_per_image > 4096) return AFI_ERR_UNSUPPORTED;
    if (ld_pred < (long long)K + 1 + 4 * (agnostic ? 1 : K)) return AFI_ERR_BAD_ARG;
    if (!ws || ws_floats < afi_roi_box_loss_ws_floats() || ((uintptr_t)ws & 7)) return AFI_ERR_WORKSPACE;
    const long long rows = (long long)N * batch_per_image;
    long long blocks = (rows + 3) / 4;
    if (blocks > ROIL_LOSS_BLOCKS) blocks = ROIL_LOSS_BLOCKS;
    const RoiLossArgs q{N, batch_per_image, K, agnostic ? 1 : 0, ld_pred, wx, wy, ww, wh, beta};
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(afi_roi_box_loss_kernel, dim3((unsigned)blocks), dim3(256), 0, st, q, pred, boxes, counts, gt_classes, gt_boxes, dpred,
                       (double*)ws);
    hipLaunchKernelGGL(afi_roi_box_loss_final_kernel, dim3(1), dim3(64), 0, st, (const double*)ws, (int)blocks, counts, N, batch_per_image, loss);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}

// ------------------------------------------------------------------------------------------------ ROIAlign backward
struct RoiBwdLevels {
    int L, min_level;
    AfiView v[ROIL_MAX_LEVELS];
    int H[ROIL_MAX_LEVELS], W[ROIL_MAX_LEVELS];
    int th[ROIL_MAX_LEVELS], tw[ROIL_MAX_LEVELS];       // tiles per column / row of a level
    long long off[ROIL_MAX_LEVELS + 1];                 // first block of a level; a level has N th tw blocks
};

// The forward's geometry of one box (afi_roi_align_kernel's expressions, fp64, no contraction).
struct RoiGeom {
    int ok, li, gh, gw, cnt;
    double sh, sw, rh, rw, binh, binw;
};
__device__ __forceinline__ RoiGeom roil_geom(const float* __restrict__ b, int min_level, int L, int S, int sr) {
#pragma clang fp contract(off)
    RoiGeom g{};
    const double x1 = (double)b[0], y1 = (double)b[1], x2 = (double)b[2], y2 = (double)b[3];
    const double bw = x2 - x1, bh = y2 - y1;
    if (!(bw > 0.0 && bh > 0.0)) return g;              // ok = 0: no samples
    const double lf = floor(ROIL_CANON_LEVEL + log2(sqrt(bw * bh) / ROIL_CANON_SIZE));
    int level = min_level;
    if (lf > (double)min_level) level = lf < (double)(min_level + L - 1) ? (int)lf : min_level + L - 1;
    g.ok = 1;
    g.li = level - min_level;
    const double scale = 1.0 / (double)(1 << level);
    g.sw = x1 * scale - 0.5; g.sh = y1 * scale - 0.5; g.rw = bw * scale; g.rh = bh * scale;
    g.binw = g.rw / (double)S; g.binh = g.rh / (double)S;
    g.gh = sr; g.gw = sr;
    if (sr <= 0) {
        const double a = ceil(g.rh / (double)S), c = ceil(g.rw / (double)S);
        g.gh = a < (double)ROIL_MAX_GRID ? (int)a : ROIL_MAX_GRID;
        g.gw = c < (double)ROIL_MAX_GRID ? (int)c : ROIL_MAX_GRID;
    }
    g.cnt = g.gh * g.gw > 1 ? g.gh * g.gw : 1;
    return g;
}

// The sum of the 1-D weights that bin p's `grid` samples along one axis give pixel `pix` (tests/roi_f64.py: _axis_weights), in sample order.
__device__ __forceinline__ double roil_axis_weight(double start, double binsz, int grid, int p, int size, int pix) {
#pragma clang fp contract(off)
    double acc = 0.0;
    for (int i = 0; i < grid; ++i) {
        double v = start + (double)p * binsz + ((double)i + 0.5) * binsz / (double)grid;
        if (v < -1.0 || v > (double)size) continue;
        if (v <= 0.0) v = 0.0;
        int lo = (int)v, hi;
        if (lo >= size - 1) { lo = hi = size - 1; v = (double)lo; } else hi = lo + 1;
        const double l = v - (double)lo;
        if (lo == pix) acc += 1.0 - l;
        if (hi == pix) acc += l;
    }
    return acc;
}

// A conservative pixel interval [lo, hi] of an axis: every sample lies inside (start, start + roi), touches floor(max(v, 0)) and the pixel after.
__device__ __forceinline__ void roil_span(double start, double roi, int size, int* lo, int* hi) {
    const double a = fmin(fmax(start, 0.0), (double)size), b = fmin(fmax(start + roi, -2.0), (double)size);
    *lo = (int)floor(a);
    *hi = (int)floor(b) + 1;
    if (*hi > size - 1) *hi = size - 1;
    if (start + roi < -1.0 || start > (double)size) { *lo = 1; *hi = 0; }     // every sample is outside [-1, size]: empty
}

// info[8 r .. 8 r + 7] of box r = n B + j: level index (-1: padding or no samples), y_lo, y_hi, x_lo, x_hi.
__global__ __launch_bounds__(256) void afi_roi_align_bwd_prep_kernel(const RoiBwdLevels lv, int N, int B, int S, int sr,
                                                                     const float* __restrict__ boxes, const int* __restrict__ counts,
                                                                     int* __restrict__ info) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= (long long)N * B) return;
    const int n = (int)(r / B), j = (int)(r - (long long)n * B);
    int li = -1, y0 = 1, y1 = 0, x0 = 1, x1 = 0;
    if (j < counts[n]) {
        const RoiGeom g = roil_geom(boxes + 4 * r, lv.min_level, lv.L, S, sr);
        if (g.ok) {
            li = g.li;
            roil_span(g.sh, g.rh, lv.H[li], &y0, &y1);
            roil_span(g.sw, g.rw, lv.W[li], &x0, &x1);
        }
    }
    int4* o = (int4*)(info + 8 * r);
    o[0] = make_int4(li, y0, y1, x0);
    o[1] = make_int4(x1, 0, 0, 0);
}

// grid (blocks of all levels, channel chunks of 64 float4).  LP: lanes per pixel (4 .. 64, a power of two >= min(C4, 64)); the block's 256
// threads cover 256 / LP pixels per pass and the tile's 64 pixels in LP / 4 passes: pixel of pass p = p (256 / LP) + tid / LP.
__global__ __launch_bounds__(256) void afi_roi_align_bwd_kernel(const RoiBwdLevels lv, int N, int B, int C4, int S, int sr, int LP,
                                                                const float* __restrict__ dpooled, const float* __restrict__ boxes,
                                                                const int* __restrict__ counts, const int* __restrict__ info) {
#pragma clang fp contract(off)
    __shared__ int hits[256];
    __shared__ int wtot[16];
    __shared__ float sWy[ROIL_MAX_S][ROIL_TILE], sWx[ROIL_MAX_S][ROIL_TILE];
    __shared__ int sLo[2][ROIL_TILE], sHi[2][ROIL_TILE];
    const int tid = threadIdx.x;
    int li = 0;
    while (li + 1 < lv.L && (long long)blockIdx.x >= lv.off[li + 1]) ++li;
    const int H = lv.H[li], W = lv.W[li], tw = lv.tw[li], th = lv.th[li];
    const int rel = (int)((long long)blockIdx.x - lv.off[li]), n = rel / (th * tw), t = rel - n * (th * tw);
    const int ty0 = (t / tw) * ROIL_TILE, tx0 = (t - (t / tw) * tw) * ROIL_TILE;
    const int sub = tid / LP, c4 = blockIdx.y * 64 + (tid - sub * LP), ppp = 256 / LP, passes = LP / 4;
    const bool lane_on = (tid - sub * LP) < 64 && c4 < C4;
    float4 acc[16];
#pragma unroll
    for (int p = 0; p < 16; ++p) acc[p] = make_float4(0.f, 0.f, 0.f, 0.f);
    int cnt_n = counts[n];
    cnt_n = cnt_n < 0 ? 0 : (cnt_n > B ? B : cnt_n);
    for (int j0 = 0; j0 < cnt_n; j0 += 256) {
        const int j = j0 + tid;
        bool hit = false;
        if (j < cnt_n) {
            const int4* q = (const int4*)(info + 8 * ((long long)n * B + j));
            const int4 a = q[0];
            const int x1 = q[1].x;
            hit = a.x == li && a.y <= ty0 + ROIL_TILE - 1 && a.z >= ty0 && a.w <= tx0 + ROIL_TILE - 1 && x1 >= tx0;
        }
        int nh;
        const int inc = rpn_block_scan(hit ? 1 : 0, wtot, &nh);
        if (hit) hits[inc - 1] = j;
        __syncthreads();
        for (int h = 0; h < nh; ++h) {
            const int jb = hits[h];
            const long long r = (long long)n * B + jb;
            // the two axis tables of this box over the tile's rows / columns: thread (axis, p, slot)
            if (tid < 2 * S * ROIL_TILE) {
                const int axis = tid / (S * ROIL_TILE), rem = tid - axis * (S * ROIL_TILE), p = rem / ROIL_TILE, slot = rem - p * ROIL_TILE;
                const RoiGeom g = roil_geom(boxes + 4 * r, lv.min_level, lv.L, S, sr);
                if (axis == 0) {
                    const double w = ty0 + slot < H ? roil_axis_weight(g.sh, g.binh, g.gh, p, H, ty0 + slot) : 0.0;
                    sWy[p][slot] = (float)(w / (double)g.cnt);
                } else {
                    const double w = tx0 + slot < W ? roil_axis_weight(g.sw, g.binw, g.gw, p, W, tx0 + slot) : 0.0;
                    sWx[p][slot] = (float)w;
                }
            }
            __syncthreads();
            if (tid < 2 * ROIL_TILE) {                       // per row / column of the tile: the first and last bin with a weight
                const int axis = tid / ROIL_TILE, slot = tid - axis * ROIL_TILE;
                int lo = S, hi = -1;
                for (int p = 0; p < S; ++p) {
                    const float w = axis == 0 ? sWy[p][slot] : sWx[p][slot];
                    if (w != 0.f) { if (lo == S) lo = p; hi = p; }
                }
                sLo[axis][slot] = lo;
                sHi[axis][slot] = hi;
            }
            __syncthreads();
            if (lane_on) {
                const float4* gp = (const float4*)dpooled + r * S * S * C4 + c4;
#pragma unroll
                for (int p = 0; p < 16; ++p) {
                    if (p < passes) {
                        const int pix = p * ppp + sub, ry = pix >> 3, rx = pix & 7;
                        const int ylo = sLo[0][ry], yhi = sHi[0][ry], xlo = sLo[1][rx], xhi = sHi[1][rx];
                        float4 a = acc[p];
                        for (int ph = ylo; ph <= yhi; ++ph) {
                            const float wy = sWy[ph][ry];
                            if (wy == 0.f) continue;
                            for (int pw = xlo; pw <= xhi; ++pw) {
                                const float wx = sWx[pw][rx];
                                if (wx == 0.f) continue;
                                const float w = wy * wx;
                                const float4 gq = gp[(long long)(ph * S + pw) * C4];
                                a.x = fmaf(w, gq.x, a.x); a.y = fmaf(w, gq.y, a.y); a.z = fmaf(w, gq.z, a.z); a.w = fmaf(w, gq.w, a.w);
                            }
                        }
                        acc[p] = a;
                    }
                }
            }
            __syncthreads();
        }
    }
    if (!lane_on) return;
    const AfiView v = lv.v[li];
    float* base = v.p + (long long)n * v.sN + 4 * (long long)c4;
#pragma unroll
    for (int p = 0; p < 16; ++p) {
        if (p < passes) {
            const int pix = p * ppp + sub, y = ty0 + (pix >> 3), x = tx0 + (pix & 7);
            if (y < H && x < W) *(float4*)(base + (long long)y * v.sH + (long long)x * v.sW) = acc[p];
        }
    }
}

long long afi_roi_align_bwd_ws_floats(int N, int batch_per_image) {
    if (N <= 0 || batch_per_image <= 0) return -1;
    return 8ll * N * batch_per_image;
}

int afi_roi_align_bwd(const float* dpooled, const afi_view_t* grads, const int* level_hw, int L, int min_level, int N, int C, const float* boxes,
                      const int* counts, int batch_per_image, int S, int sampling_ratio, float* ws, long long ws_floats, void* stream) {
    if (!dpooled || !grads || !level_hw || !boxes || !counts || L <= 0 || min_level < 0 || N <= 0 || N > 65535 || C <= 0 || batch_per_image <= 0 ||
        S <= 0 || sampling_ratio < 0)
        return AFI_ERR_BAD_ARG;
    if (L > ROIL_MAX_LEVELS || min_level + L - 1 > 30 || (C & 3) || S > ROIL_MAX_S || sampling_ratio > ROIL_MAX_GRID || ((uintptr_t)dpooled & 15) ||
        ((uintptr_t)boxes & 3))
        return AFI_ERR_UNSUPPORTED;
    if (!ws || ws_floats < afi_roi_align_bwd_ws_floats(N, batch_per_image) || ((uintptr_t)ws & 15)) return AFI_ERR_WORKSPACE;
    RoiBwdLevels lv{};
    lv.L = L;
    lv.min_level = min_level;
    long long off = 0;
    for (int l = 0; l < ROIL_MAX_LEVELS; ++l) {
        lv.off[l] = off;
        const int s = l < L ? l : L - 1;
        const afi_view_t& q = grads[s];
        if (!q.p || level_hw[2 * s] <= 0 || level_hw[2 * s + 1] <= 0) return AFI_ERR_BAD_ARG;
        if (((uintptr_t)q.p & 15) || (q.sN & 3) || (q.sH & 3) || (q.sW & 3)) return AFI_ERR_UNSUPPORTED;
        lv.v[l] = AfiView{(float*)q.p, q.sN, q.sH, q.sW};
        lv.H[l] = level_hw[2 * s];
        lv.W[l] = level_hw[2 * s + 1];
        lv.th[l] = (lv.H[l] + ROIL_TILE - 1) / ROIL_TILE;
        lv.tw[l] = (lv.W[l] + ROIL_TILE - 1) / ROIL_TILE;
        if (l < L) off += (long long)N * lv.th[l] * lv.tw[l];
    }
    lv.off[ROIL_MAX_LEVELS] = off;
    if (off > 0x7fffffffll) return AFI_ERR_UNSUPPORTED;
    const int C4 = C / 4;
    int LP = 4;
    while (LP < 64 && LP < C4) LP <<= 1;
    const int chunks = (C4 + 63) / 64;
    hipStream_t st = (hipStream_t)stream;
    const long long rows = (long long)N * batch_per_image;
    hipLaunchKernelGGL(afi_roi_align_bwd_prep_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, lv, N, batch_per_image, S,
                       sampling_ratio, boxes, counts, (int*)ws);
    hipLaunchKernelGGL(afi_roi_align_bwd_kernel, dim3((unsigned)off, chunks), dim3(256), 0, st, lv, N, batch_per_image, C4, S, sampling_ratio, LP,
                       dpooled, boxes, counts, (const int*)ws);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}
