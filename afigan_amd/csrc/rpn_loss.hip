// The training side of the RPN (afigan_amd/rpn.py: RPN.losses): detectron2 v0.1.1's RPNOutputs._get_ground_truth, Matcher, subsample_labels,
// Box2BoxTransform.get_deltas and rpn_losses, over anchors that are never materialised -- anchor (y W + x) A + a of a level is its cell anchor
// plus (x stride, y stride), each coordinate one fp32 addition, formed from the index as afi_rpn_decode does.  The levels of an image are
// concatenated in IN_FEATURES order; R = all anchors of an image, at most 2^22.
//   afi_rpn_match    two sweeps over the anchors, one thread per anchor, the image's ground-truth boxes in LDS in tiles of 256.
//                    Sweep 1: the IoU with every box (afi_box_match.h: fp32, no contraction), the running (max, lowest index) per anchor and
//                    the threshold label; best[g] = max IoU of box g over all anchors, reduced per block in LDS and merged across blocks by an
//                    integer atomicMax on the bit pattern (IoUs are non-negative, so the patterns order as the numbers do; a maximum does not
//                    depend on the order of its merges).  Sweep 2 computes the same IoUs again -- same inputs, same operations, same bits --
//                    and gives label 1 to every anchor whose IoU with some box EQUALS that box's best (detectron2's low-quality matches;
//                    matched_idx stays).  A box with best 0 promotes every anchor that does not overlap it, as the reference does.
//                    No G x R array exists: 4 R bytes + the boxes read per sweep, 5 R (+ R) bytes written.
//   afi_rpn_sample   per image and class (positive, negative) one block: the class's count, then a radix select of the `need` smallest
//                    (key, anchor index) pairs on the words ~key << 22 | ~index (afi_rpn_topk's scheme: the k LARGEST of distinct words),
//                    then one ordered sweep that relabels the rest -1 and emits the sampled anchors in ascending index (block prefix sum).
//                    The histogram atomics only count.  A pure function of labels and keys.
//   afi_rpn_loss     one block over the N x B sampled anchors of all levels: gather logit and deltas from the pixel-major head outputs, the
//                    regression target in fp64 from the fp32 anchor and box, rounded once; the per-anchor terms in fp32; their sums in fp64
//                    (each thread its entries in order, a wavefront shuffle tree, the waves in order); the gradient of both scaled losses
//                    with respect to the head output, stored at the sampled anchors only (the caller zero-fills).
// Nothing here synchronises with the host; every output is bit-identical from run to run.
#include "../../include/afigan_hip.h"
#include "afi_common.h"
#include "afi_select.h"
#include "afi_box_match.h"

#define RPNL_MAX_A 16
#define RPNL_MAX_LEVELS 8
#define RPNL_IDX_BITS 22
#define RPNL_IDX_MASK 0x3FFFFFu
#define RPNL_MAX_R (1 << RPNL_IDX_BITS)
#define RPNL_GT_TILE 256           // ground-truth boxes per LDS tile
#define RPNL_MAX_GT 1024           // boxes per image (four tiles)
#define RPNL_MAX_BATCH 4096        // BATCH_SIZE_PER_IMAGE

struct RpnTrainLevels { int L, A; int off[RPNL_MAX_LEVELS + 1]; int H[RPNL_MAX_LEVELS], W[RPNL_MAX_LEVELS], stride[RPNL_MAX_LEVELS]; };
struct RpnTrainViews { AfiView v[RPNL_MAX_LEVELS]; };

// Where global anchor i lives: level l, pixel (y, x), cell anchor a.
struct RpnAnchorAt { int l, y, x, a; };
__device__ __forceinline__ RpnAnchorAt rpn_anchor_at(const RpnTrainLevels& lv, int i) {
    int l = 0;
    while (l + 1 < lv.L && i >= lv.off[l + 1]) ++l;
    const int j = i - lv.off[l], pix = j / lv.A, a = j - pix * lv.A, y = pix / lv.W[l], x = pix - y * lv.W[l];
    return RpnAnchorAt{l, y, x, a};
}
// cell: [L][A][4] fp32.  DefaultAnchorGenerator adds the fp32 shift to the fp32 cell anchor: one rounding per coordinate.
__device__ __forceinline__ float4 rpn_anchor_box(const RpnTrainLevels& lv, const float* __restrict__ cell, const RpnAnchorAt p) {
    const float* c = cell + ((long long)p.l * lv.A + p.a) * 4;
    const float sx = (float)(p.x * lv.stride[p.l]), sy = (float)(p.y * lv.stride[p.l]);
    return make_float4(c[0] + sx, c[1] + sy, c[2] + sx, c[3] + sy);
}

static int rpn_train_levels(const int* level_hw, const int* strides, int L, int A, RpnTrainLevels* out) {
    if (!level_hw || !strides || L <= 0 || A <= 0) return AFI_ERR_BAD_ARG;
    if (L > RPNL_MAX_LEVELS || A > RPNL_MAX_A) return AFI_ERR_UNSUPPORTED;
    RpnTrainLevels lv{};
    lv.L = L; lv.A = A;
    long long off = 0;
    for (int l = 0; l < RPNL_MAX_LEVELS; ++l) {
        lv.off[l] = (int)off;
        if (l < L) {
            const int H = level_hw[2 * l], W = level_hw[2 * l + 1];
            if (H <= 0 || W <= 0 || strides[l] <= 0) return AFI_ERR_BAD_ARG;
            lv.H[l] = H; lv.W[l] = W; lv.stride[l] = strides[l];
            off += (long long)H * W * A;
            if (off > RPNL_MAX_R) return AFI_ERR_UNSUPPORTED;
        } else {
            lv.H[l] = 1; lv.W[l] = 1; lv.stride[l] = 1;
        }
    }
    lv.off[RPNL_MAX_LEVELS] = (int)off;
    for (int l = L; l <= RPNL_MAX_LEVELS; ++l) lv.off[l] = (int)off;
    *out = lv;
    return AFI_OK;
}

// ------------------------------------------------------------------------------------------------ match
__global__ __launch_bounds__(256) void afi_rpn_match_zero_kernel(unsigned* __restrict__ p, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = 0u;
}

// SWEEP 1: labels by threshold, matched_idx, best[].  SWEEP 2: promotion of the anchors that tie a box's best.
template <int SWEEP>
__global__ __launch_bounds__(256) void afi_rpn_match_kernel(const RpnTrainLevels lv, const float* __restrict__ cell, const float* __restrict__ gt,
                                                            const int* __restrict__ counts, int Gmax, float t0, float t1,
                                                            unsigned* __restrict__ best, signed char* __restrict__ labels,
                                                            int* __restrict__ matched_idx) {
    __shared__ float4 sb[RPNL_GT_TILE];
    __shared__ float sa[RPNL_GT_TILE];
    __shared__ unsigned sbest[RPNL_GT_TILE];
    const int img = blockIdx.y, tid = threadIdx.x, R = lv.off[lv.L], i = blockIdx.x * 256 + tid;
    int G = counts[img];
    G = G < 0 ? 0 : (G > Gmax ? Gmax : G);
    const bool live = i < R;
    float4 an = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live) an = rpn_anchor_box(lv, cell, rpn_anchor_at(lv, i));
    const float aarea = afi_box_area(an);
    AfiMatch m{0.f, 0};
    bool promote = false;
    for (int g0 = 0; g0 < G; g0 += RPNL_GT_TILE) {
        const int nt = G - g0 < RPNL_GT_TILE ? G - g0 : RPNL_GT_TILE;
        if (tid < nt) {
            const long long o = (long long)img * Gmax + g0 + tid;
            const float* q = gt + 4 * o;
            const float4 b = make_float4(q[0], q[1], q[2], q[3]);
            sb[tid] = b;
            sa[tid] = afi_box_area(b);
            sbest[tid] = SWEEP == 1 ? 0u : best[o];
        }
        __syncthreads();
        if (live) {
            for (int j = 0; j < nt; ++j) {
                const float iou = afi_box_iou(sb[j], sa[j], an, aarea);
                if (SWEEP == 1) {
                    afi_match_update(m, iou, g0 + j);
                    if (iou > 0.f) atomicMax(&sbest[j], __float_as_uint(iou));
                } else {
                    promote = promote || (iou == __uint_as_float(sbest[j]));
                }
            }
        }
        __syncthreads();
        if (SWEEP == 1 && tid < nt && sbest[tid]) atomicMax(&best[(long long)img * Gmax + g0 + tid], sbest[tid]);
        __syncthreads();
    }
    if (!live) return;
    const long long o = (long long)img * R + i;
    if (SWEEP == 1) {
        labels[o] = (signed char)(G > 0 ? afi_match_label(m.val, t0, t1) : 0);
        matched_idx[o] = m.idx;
    } else if (promote) {
        labels[o] = 1;
    }
}

int afi_rpn_match(const int* level_hw, const int* strides, int L, int A, const float* cell_anchors, int N, const float* gt, const int* counts,
                  int Gmax, float t0, float t1, signed char* labels, int* matched_idx, float* ws, long long ws_floats, void* stream) {
    RpnTrainLevels lv;
    AFI_TRY(rpn_train_levels(level_hw, strides, L, A, &lv));
    if (!cell_anchors || !gt || !counts || !labels || !matched_idx || N <= 0 || N > 65535 || Gmax <= 0 || !(t0 <= t1)) return AFI_ERR_BAD_ARG;
    if (Gmax > RPNL_MAX_GT) return AFI_ERR_UNSUPPORTED;
    if (!ws || ws_floats < (long long)N * Gmax) return AFI_ERR_WORKSPACE;
    unsigned* best = (unsigned*)ws;
    hipStream_t st = (hipStream_t)stream;
    const int R = lv.off[L];
    const dim3 grid((R + 255) / 256, N);
    hipLaunchKernelGGL(afi_rpn_match_zero_kernel, dim3((N * Gmax + 255) / 256), dim3(256), 0, st, best, N * Gmax);
    hipLaunchKernelGGL(afi_rpn_match_kernel<1>, grid, dim3(256), 0, st, lv, cell_anchors, gt, counts, Gmax, t0, t1, best, labels, matched_idx);
    hipLaunchKernelGGL(afi_rpn_match_kernel<2>, grid, dim3(256), 0, st, lv, cell_anchors, gt, counts, Gmax, t0, t1, best, labels, matched_idx);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}

// ------------------------------------------------------------------------------------------------ sample
// The larger word is the EARLIER pick: smaller key first, equal keys in ascending anchor index.  Distinct for distinct i < 2^22.
__device__ __forceinline__ u64 rpn_sample_word(unsigned key, int i) {
    return ((u64)(~key) << RPNL_IDX_BITS) | (u64)((~(unsigned)i) & RPNL_IDX_MASK);
}

// grid (2, N): block x = 0 samples the positives (label 1) of image y, x = 1 the negatives (label 0).  labels_out must not alias labels_in:
// the two blocks of an image read all of labels_in while each writes its own part of labels_out.
__global__ __launch_bounds__(1024) void afi_rpn_sample_kernel(const signed char* __restrict__ labels_in, const unsigned* __restrict__ keys, int R,
                                                              int B, int P, signed char* __restrict__ labels_out, int* __restrict__ sidx,
                                                              int* __restrict__ n_pos, int* __restrict__ n_neg) {
    __shared__ int hist[2048];
    __shared__ int wtot[16];
    __shared__ int res[2];
    const int img = blockIdx.y, tid = threadIdx.x, cls = blockIdx.x == 0 ? 1 : 0;
    const signed char* lab = labels_in + (long long)img * R;
    const unsigned* key = keys + (long long)img * R;
    int cp = 0, cn = 0;
    for (int i = tid; i < R; i += 1024) {
        const int l = lab[i];
        cp += l == 1;
        cn += l == 0;
    }
    int tp, tn;
    rpn_block_scan(cp, wtot, &tp);
    __syncthreads();
    rpn_block_scan(cn, wtot, &tn);
    __syncthreads();
    const int npos = tp < P ? tp : P, nneg = tn < B - npos ? tn : B - npos;
    const int m = cls ? tp : tn, want = cls ? npos : nneg, base = cls ? 0 : npos;
    auto word = [&](int i, u64* c) {                    // the members of this block's class take part
        if (lab[i] != cls) return false;
        *c = rpn_sample_word(key[i], i);
        return true;
    };
    const RpnCut cut = rpn_radix_select(word, R, m, want, RPNL_IDX_BITS, hist, wtot, res);
    // the members whose word, cut at cut.shift, is at or above the prefix: exactly `want` of them (all of them when want == m, none when 0)
    signed char* out = labels_out + (long long)img * R;
    int* list = sidx + (long long)img * B;
    int run = 0;
    for (int c0 = 0; c0 < R; c0 += 1024) {
        const int i = c0 + tid;
        const int l = i < R ? (int)lab[i] : -2;
        const bool member = l == cls;
        const bool s = member && want > 0 && (rpn_sample_word(key[i], i) >> cut.shift) >= cut.prefix;
        int tot;
        const int inc = rpn_block_scan(s ? 1 : 0, wtot, &tot);
        if (s) {
            const int pos = run + inc - 1;
            if (pos < want) list[base + pos] = i;
        }
        if (member) out[i] = (signed char)(s ? cls : -1);
        else if (cls == 1 && i < R && l != 0) out[i] = (signed char)-1;     // the ignored anchors pass through the positives' block
        run += tot;
        __syncthreads();
    }
    if (cls == 0) {
        for (int j = npos + nneg + tid; j < B; j += 1024) list[j] = -1;
        if (tid == 0) { n_pos[img] = npos; n_neg[img] = nneg; }
    }
}

int afi_rpn_sample(const signed char* labels, const unsigned int* keys, int N, long long R, int batch_per_image, int num_pos_max,
                   signed char* labels_out, int* sampled_idx, int* n_pos, int* n_neg, void* stream) {
    if (!labels || !keys || !labels_out || !sampled_idx || !n_pos || !n_neg || N <= 0 || N > 65535 || R <= 0 || batch_per_image <= 0 ||
        num_pos_max < 0 || num_pos_max > batch_per_image || labels == labels_out)
        return AFI_ERR_BAD_ARG;
    if (R > RPNL_MAX_R || batch_per_image > RPNL_MAX_BATCH) return AFI_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(afi_rpn_sample_kernel, dim3(2, N), dim3(1024), 0, (hipStream_t)stream, labels, (const unsigned*)keys, (int)R,
                       batch_per_image, num_pos_max, labels_out, sampled_idx, n_pos, n_neg);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}

// ------------------------------------------------------------------------------------------------ loss
struct RpnLossArgs {
    int N, B, Gmax;
    float wx, wy, ww, wh, beta;
    double scale_cls, scale_loc;
};

__device__ __forceinline__ double rpn_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;                                           // lane 0: the wavefront's sum, one fixed tree
}

__global__ __launch_bounds__(256) void afi_rpn_loss_kernel(const RpnTrainLevels lv, const RpnTrainViews heads, const RpnTrainViews grads,
                                                           const float* __restrict__ cell, const RpnLossArgs q, const float* __restrict__ gt,
                                                           const int* __restrict__ matched_idx, const int* __restrict__ sidx,
                                                           const int* __restrict__ n_pos, const int* __restrict__ n_neg,
                                                           float* __restrict__ loss) {
    __shared__ double wsum[2][4];
    const int tid = threadIdx.x, R = lv.off[lv.L], A = lv.A;
    const float gs_cls = (float)q.scale_cls, gs_loc = (float)q.scale_loc;
    double acc_cls = 0.0, acc_loc = 0.0;
    for (int e = tid; e < q.N * q.B; e += 256) {
        const int img = e / q.B, j = e - img * q.B;
        const int np = n_pos[img], nn = n_neg[img];
        if (j >= np + nn) continue;
        const int i = sidx[e];
        if (i < 0 || i >= R) continue;
        const bool pos = j < np;
        const RpnAnchorAt at = rpn_anchor_at(lv, i);
        const AfiView hv = heads.v[at.l], gv = grads.v[at.l];
        const long long po = (long long)img * hv.sN + (long long)at.y * hv.sH + (long long)at.x * hv.sW;
        const long long go = (long long)img * gv.sN + (long long)at.y * gv.sH + (long long)at.x * gv.sW;
        // objectness: max(z, 0) - z t + log1p(exp(-|z|)), d/dz = sigmoid(z) - t
        const float z = hv.p[po + at.a], t = pos ? 1.f : 0.f;
        const float ez = expf(-fabsf(z));
        acc_cls += (double)(fmaxf(z, 0.f) - z * t + log1pf(ez));
        const float sg = z >= 0.f ? 1.f / (1.f + ez) : ez / (1.f + ez);
        gv.p[go + at.a] = (sg - t) * gs_cls;
        if (!pos) continue;
        // Box2BoxTransform.get_deltas(anchor, matched box) in fp64 from the fp32 coordinates, rounded once
        int g = matched_idx[(long long)img * R + i];
        g = g < 0 ? 0 : (g >= q.Gmax ? q.Gmax - 1 : g);
        const float4 an = rpn_anchor_box(lv, cell, at);
        const float* b = gt + ((long long)img * q.Gmax + g) * 4;
        const double sw = (double)an.z - (double)an.x, sh = (double)an.w - (double)an.y;
        const double scx = (double)an.x + 0.5 * sw, scy = (double)an.y + 0.5 * sh;
        const double tw = (double)b[2] - (double)b[0], th = (double)b[3] - (double)b[1];
        const double tcx = (double)b[0] + 0.5 * tw, tcy = (double)b[1] + 0.5 * th;
        float tgt[4];
        tgt[0] = (float)((double)q.wx * (tcx - scx) / sw);
        tgt[1] = (float)((double)q.wy * (tcy - scy) / sh);
        tgt[2] = (float)((double)q.ww * log(tw / sw));
        tgt[3] = (float)((double)q.wh * log(th / sh));
        const float* pd = hv.p + po + A + 4 * at.a;
        float* gd = gv.p + go + A + 4 * at.a;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float d = pd[c] - tgt[c], ad = fabsf(d);
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
            gd[c] = gr * gs_loc;
        }
    }
    acc_cls = rpn_wave_sum(acc_cls);
    acc_loc = rpn_wave_sum(acc_loc);
    if ((tid & 63) == 0) { wsum[0][tid >> 6] = acc_cls; wsum[1][tid >> 6] = acc_loc; }
    __syncthreads();
    if (tid == 0) {
        loss[0] = (float)((((wsum[0][0] + wsum[0][1]) + wsum[0][2]) + wsum[0][3]) * q.scale_cls);
        loss[1] = (float)((((wsum[1][0] + wsum[1][1]) + wsum[1][2]) + wsum[1][3]) * q.scale_loc);
    }
}

int afi_rpn_loss(const afi_view_t* heads, const afi_view_t* grads, const int* level_hw, const int* strides, int L, int A,
                 const float* cell_anchors, int N, const float* gt, int Gmax, const int* matched_idx, const int* sampled_idx, int batch_per_image,
                 const int* n_pos, const int* n_neg, float wx, float wy, float ww, float wh, float beta, double scale_cls, double scale_loc,
                 float* loss, void* stream) {
    RpnTrainLevels lv;
    AFI_TRY(rpn_train_levels(level_hw, strides, L, A, &lv));
    if (!heads || !grads || !cell_anchors || !gt || !matched_idx || !sampled_idx || !n_pos || !n_neg || !loss || N <= 0 || N > 65535 || Gmax <= 0 ||
        batch_per_image <= 0 || !(beta >= 0.f) || !(wx > 0.f) || !(wy > 0.f) || !(ww > 0.f) || !(wh > 0.f))
        return AFI_ERR_BAD_ARG;
    if (Gmax > RPNL_MAX_GT || batch_per_image > RPNL_MAX_BATCH) return AFI_ERR_UNSUPPORTED;
    RpnTrainViews hv{}, gv{};
    for (int l = 0; l < L; ++l) {
        if (!heads[l].p || !grads[l].p) return AFI_ERR_BAD_ARG;
        hv.v[l] = AfiView{(float*)heads[l].p, heads[l].sN, heads[l].sH, heads[l].sW};
        gv.v[l] = AfiView{(float*)grads[l].p, grads[l].sN, grads[l].sH, grads[l].sW};
    }
    const RpnLossArgs q{N, batch_per_image, Gmax, wx, wy, ww, wh, beta, scale_cls, scale_loc};
    hipLaunchKernelGGL(afi_rpn_loss_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, lv, hv, gv, cell_anchors, q, gt, matched_idx, sampled_idx,
                       n_pos, n_neg, loss);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}
