// The selection stages of the frozen RPN proposal generator (afigan_amd/rpn.py); its head (3x3 conv + ReLU, the two 1x1 convs as one) runs on
// afi_conv3x3_wino_infer / afi_conv3x3_fwd and afi_conv1x1_fwd.
//   afi_rpn_topk     per image, the k highest of the H W A objectness logits of one level, sorted by (logit descending, anchor index ascending).
//                    A select, not a sort: every logit becomes an order-preserving 32-bit key, key and anchor index one 54-bit word
//                    (key << 22 | ~index: distinct words, so "the k largest words" is one well-defined set), and the k-th largest word is found
//                    by radix passes over LDS histograms (digits of 11, 11, 10 key bits, then 11, 11 index bits; the passes stop as soon as
//                    the open digit group is taken whole -- with distinct logits after the key bits).  Maps of more than 16384 logits first
//                    go through a histogram of the top 12 key bits over the whole grid and a filter that keeps the words of the bins down to
//                    the one holding the cut (typically a few thousand); one block per image then selects among those.  The <= 1024 survivors
//                    are sorted in LDS (bitonic, on the distinct words).  The integer atomics only count or hand out slots of an unordered
//                    list: the result does not depend on their order.
//   afi_rpn_decode   the selected anchors' deltas gathered from the pixel-major head output, the anchor formed from its index and the [A][4] cell
//                    anchors, Box2BoxTransform.apply_deltas (evaluated in fp64 from the fp32 inputs, rounded once), the clip to the image's own
//                    size and the MIN_SIZE test on the stored fp32 box.
//   afi_rpn_nms      greedy NMS of <= 1024 sorted boxes per image: the suppression bit matrix (a wave's 64-bit __ballot is one word, 16 words per
//                    row) is built in LDS by all sixteen waves; one wave then sweeps it 64 rows at a time -- the 64 x 64 diagonal block is
//                    resolved in registers by lane reads, the kept rows' words OR-ed into the running mask by all lanes.  The overlap test
//                    is compiled without fused multiply-adds: inter / (area_a + area_b - inter) > thresh, each operation rounded to fp32.
//   afi_rpn_merge    the kept boxes of all levels of an image in (logit descending, level, rank) order, cut to post_k: every level's list is
//                    already sorted, so an entry's place is its own rank plus one binary search per other level.  No sort, no atomics.
// The "wide" forms (lists of 1025 .. 4096 per level: PRE_NMS_TOPK_TRAIN of the reference's base config is 2000):
//   afi_rpn_topk_wide   afi_rpn_topk's kernels, the pick instantiated with sel[4096]: it sorts the next power of two >= k.
//   afi_rpn_nms_wide    the bit matrix in a workspace, its upper triangle built by one block per 64 x 64 tile; one wave per image sweeps it.
//                       The overlap test and the diagonal resolve are afi_rpn_nms's (afi_select.h).
//   afi_rpn_merge_wide  afi_rpn_merge's kernel instantiated for 5 x 4096 entries in all.
// Nothing here synchronises with the host, and every result is bit-identical from run to run and under hipGraph replay.
#include "../../include/afigan_hip.h"
#include "afi_common.h"
#include "afi_select.h"

#define RPN_MAX_A 16
#define RPN_IDX_BITS 22
#define RPN_IDX_MASK 0x3FFFFFu
#define RPN_DIRECT_MAX 16384       // up to here the selecting block reads the logits itself
#define RPN_BINS 4096              // grid histogram: the top 12 key bits
#define RPN_HDR 4104               // ints per image in front of the candidate lists: the histogram, the list length, padding to 8 bytes
#define RPN_MAX_LEVELS 8

struct RpnLevels { int L; int off[RPN_MAX_LEVELS + 1]; };

// Order-preserving key: a < b <=> key(a) < key(b) for numbers, -0 and +0 share one key (they compare equal), NaN is 0, below every number
// (-inf is 0x007fffff).
__device__ __forceinline__ unsigned rpn_key(float v) {
    if (v != v) return 0u;
    if (v == 0.f) return 0x80000000u;
    const unsigned b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ const float* rpn_at(const AfiView& v, int img, int i, int W, int A) {
    const int pix = i / A, a = i - pix * A, y = pix / W, x = pix - y * W;
    return v.p + (long long)img * v.sN + (long long)y * v.sH + (long long)x * v.sW + a;
}

__device__ __forceinline__ u64 rpn_word(float v, int i) { return ((u64)rpn_key(v) << RPN_IDX_BITS) | (u64)((~(unsigned)i) & RPN_IDX_MASK); }

// ------------------------------------------------------------------------------------------------ top-k: grid histogram and filter (large maps)
__global__ __launch_bounds__(256) void afi_rpn_zero_kernel(int* __restrict__ p, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = 0;
}

__global__ __launch_bounds__(256) void afi_rpn_hist_kernel(const AfiView lg, int W, int A, int n, int* __restrict__ hdr) {
    __shared__ int h[RPN_BINS];
    const int img = blockIdx.y;
    for (int i = threadIdx.x; i < RPN_BINS; i += 256) h[i] = 0;
    __syncthreads();
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) atomicAdd(&h[rpn_key(*rpn_at(lg, img, i, W, A)) >> 20], 1);
    __syncthreads();
    int* g = hdr + (long long)img * RPN_HDR;
    for (int i = threadIdx.x; i < RPN_BINS; i += 256)
        if (h[i]) atomicAdd(&g[i], h[i]);
}

__global__ __launch_bounds__(256) void afi_rpn_filter_kernel(const AfiView lg, int W, int A, int n, int k, int* __restrict__ hdr,
                                                             u64* __restrict__ cand_all) {
    __shared__ int h[RPN_BINS];
    __shared__ int wtot[16];
    __shared__ int res[2];
    const int img = blockIdx.y, lane = threadIdx.x & 63;
    int* g = hdr + (long long)img * RPN_HDR;
    for (int i = threadIdx.x; i < RPN_BINS; i += 256) h[i] = g[i];
    __syncthreads();
    rpn_find_digit(h, RPN_BINS, k, wtot, res);
    const unsigned cut = (unsigned)res[0];
    u64* cand = cand_all + (long long)img * n;
    for (int i0 = blockIdx.x * 256; i0 < n; i0 += gridDim.x * 256) {
        const int i = i0 + threadIdx.x;
        u64 c = 0;
        bool take = false;
        if (i < n) {
            c = rpn_word(*rpn_at(lg, img, i, W, A), i);
            take = (unsigned)(c >> (RPN_IDX_BITS + 20)) >= cut;
        }
        const u64 m = __ballot(take);
        if (m) {
            const int first = __ffsll((long long)m) - 1;
            int base = 0;
            if (lane == first) base = atomicAdd(&g[RPN_BINS], __popcll(m));
            base = __shfl(base, first, 64);
            const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
            if (take && pos < n) cand[pos] = c;
        }
    }
}

// ------------------------------------------------------------------------------------------------ top-k: select k of m words, sort, write
// DIRECT: the m = n words are formed from the logits; else they are the filter's list (hdr[RPN_BINS] of them).  One block per image, k <= MAXK
// (RPN_MAXK or RPN_MAXK_WIDE).  The selected words are sorted in LDS (bitonic): P = 1024 words for RPN_MAXK, a thread per word; 2048 or 4096
// for RPN_MAXK_WIDE, P / 2 compare-exchanges per step over the 1024 threads.  The words are distinct apart from the zero padding.
template <bool DIRECT, int MAXK>
__global__ __launch_bounds__(1024) void afi_rpn_pick_kernel(const AfiView lg, int W, int A, int n, int k, const int* __restrict__ hdr,
                                                            const u64* __restrict__ cand_all, float* __restrict__ vals, int* __restrict__ idx,
                                                            long long ld) {
    __shared__ int hist[2048];
    __shared__ int wtot[16];
    __shared__ int res[2];
    __shared__ u64 sel[MAXK];
    __shared__ int nsel;
    const int img = blockIdx.x, tid = threadIdx.x;
    int m = n;
    const u64* cand = nullptr;
    if (!DIRECT) {
        m = hdr[(long long)img * RPN_HDR + RPN_BINS];
        m = m < 0 ? 0 : (m > n ? n : m);
        cand = cand_all + (long long)img * n;
    }
    auto word = [&](int i) -> u64 { return DIRECT ? rpn_word(*rpn_at(lg, img, i, W, A), i) : cand[i]; };
    const RpnCut cut = rpn_radix_select([&](int i, u64* c) { *c = word(i); return true; }, m, m, k < m ? k : m, RPN_IDX_BITS, hist, wtot, res);
    // the words above the open group and the group itself (taken whole): min(k, m) words
    if (tid == 0) nsel = 0;
    __syncthreads();
    for (int i = tid; i < m; i += 1024) {
        const u64 c = word(i);
        if ((c >> cut.shift) >= cut.prefix) {
            const int s = atomicAdd(&nsel, 1);
            if (s < MAXK) sel[s] = c;                      // (never more than min(k, m) <= MAXK: the guard keeps a wrong count inside the array)
        }
    }
    __syncthreads();
    const int ns = nsel < MAXK ? nsel : MAXK;
    const int P = (MAXK > RPN_MAXK && k <= MAXK / 2 && ns <= MAXK / 2) ? MAXK / 2 : MAXK;
    for (int i = ns + tid; i < P; i += 1024) sel[i] = 0;   // below every real word (a real word's index field is never all ones: n <= RPN_IDX_MASK)
    __syncthreads();
    for (int ksz = 2; ksz <= P; ksz <<= 1)
        for (int j = ksz >> 1; j > 0; j >>= 1) {
            if constexpr (MAXK == RPN_MAXK) {              // P = the block: a thread per word, the lower word's thread exchanges the pair
                const int o = tid ^ j;                     // (the inference path's sort; the pair form with half the threads idle was
                if (o > tid) {                             // measured beside it: DESIGN 25)
                    const u64 a = sel[tid], b = sel[o];
                    const bool desc = (tid & ksz) == 0;
                    if (desc ? a < b : a > b) { sel[tid] = b; sel[o] = a; }
                }
            } else {
                for (int t = tid; t < (P >> 1); t += 1024) {
                    const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), o = i | j;    // the t-th pair of this step: bit j clear / set
                    const u64 a = sel[i], b = sel[o];
                    const bool desc = (i & ksz) == 0;
                    if (desc ? a < b : a > b) { sel[i] = b; sel[o] = a; }
                }
            }
            __syncthreads();
        }
    for (int t = tid; t < k; t += 1024) {
        const u64 c = sel[t];
        int i = (int)((~(unsigned)c) & RPN_IDX_MASK);
        if (c == 0 || i >= n) i = 0;                       // (never: k <= m real words)
        idx[(long long)img * ld + t] = i;
        vals[(long long)img * ld + t] = *rpn_at(lg, img, i, W, A);
    }
}

long long afi_rpn_topk_ws_floats(int N, int H, int W, int A) {
    if (N <= 0 || H <= 0 || W <= 0 || A <= 0 || A > RPN_MAX_A) return -1;
    const long long n = (long long)H * W * A;
    if (n >= RPN_IDX_MASK) return -1;
    if (n <= RPN_DIRECT_MAX) return 0;
    return (long long)N * RPN_HDR + 2 * (long long)N * n;
}

long long afi_rpn_topk_wide_ws_floats(int N, int H, int W, int A) { return afi_rpn_topk_ws_floats(N, H, W, A); }

// k_above < k <= MAXK: afi_rpn_topk is (0, RPN_MAXK], afi_rpn_topk_wide (RPN_MAXK, RPN_MAXK_WIDE] -- a k of the other's range is refused.
template <int MAXK>
static int rpn_topk_launch(int k_above, afi_view_t logits, int N, int H, int W, int A, int k, float* vals, int* idx, long long ld, float* ws,
                           long long ws_floats, void* stream) {
    if (!logits.p || !vals || !idx || N <= 0 || N > 65535 || H <= 0 || W <= 0 || A <= 0 || k <= 0 || ld < k) return AFI_ERR_BAD_ARG;
    const long long nn = (long long)H * W * A;
    if (A > RPN_MAX_A || k <= k_above || k > MAXK || nn >= RPN_IDX_MASK) return AFI_ERR_UNSUPPORTED;
    if (k > nn) return AFI_ERR_BAD_ARG;
    const int n = (int)nn;
    const AfiView lg{(float*)logits.p, logits.sN, logits.sH, logits.sW};
    hipStream_t st = (hipStream_t)stream;
    if (n <= RPN_DIRECT_MAX) {
        hipLaunchKernelGGL((afi_rpn_pick_kernel<true, MAXK>), dim3(N), dim3(1024), 0, st, lg, W, A, n, k, (const int*)nullptr, (const u64*)nullptr,
                           vals, idx, ld);
        return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
    }
    const long long need = afi_rpn_topk_ws_floats(N, H, W, A);
    if (!ws || ws_floats < need || ((uintptr_t)ws & 7)) return AFI_ERR_WORKSPACE;
    int* hdr = (int*)ws;
    u64* cand = (u64*)(hdr + (long long)N * RPN_HDR);          // N * RPN_HDR ints: a multiple of 8 bytes
    hipLaunchKernelGGL(afi_rpn_zero_kernel, dim3((N * RPN_HDR + 255) / 256), dim3(256), 0, st, hdr, N * RPN_HDR);      // histograms, list lengths
    int gx = (n + 256 * 8 - 1) / (256 * 8);
    if (gx > 512) gx = 512;
    hipLaunchKernelGGL(afi_rpn_hist_kernel, dim3(gx, N), dim3(256), 0, st, lg, W, A, n, hdr);
    hipLaunchKernelGGL(afi_rpn_filter_kernel, dim3(gx, N), dim3(256), 0, st, lg, W, A, n, k, hdr, cand);
    hipLaunchKernelGGL((afi_rpn_pick_kernel<false, MAXK>), dim3(N), dim3(1024), 0, st, lg, W, A, n, k, (const int*)hdr, (const u64*)cand, vals,
                       idx, ld);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}

int afi_rpn_topk(afi_view_t logits, int N, int H, int W, int A, int k, float* vals, int* idx, long long ld, float* ws, long long ws_floats,
                 void* stream) {
    return rpn_topk_launch<RPN_MAXK>(0, logits, N, H, W, A, k, vals, idx, ld, ws, ws_floats, stream);
}

int afi_rpn_topk_wide(afi_view_t logits, int N, int H, int W, int A, int k, float* vals, int* idx, long long ld, float* ws, long long ws_floats,
                      void* stream) {
    return rpn_topk_launch<RPN_MAXK_WIDE>(RPN_MAXK, logits, N, H, W, A, k, vals, idx, ld, ws, ws_floats, stream);
}

// ------------------------------------------------------------------------------------------------ decode
struct RpnDecode {
    int N, H, W, A, k, stride;
    float wx, wy, ww, wh;
    double clamp;
    float min_size;
};

__global__ __launch_bounds__(256) void afi_rpn_decode_kernel(const AfiView dl, const RpnDecode d, const float* __restrict__ cell,
                                                             const int* __restrict__ idx, long long ld, const float* __restrict__ image_hw,
                                                             float* __restrict__ boxes, int* __restrict__ valid) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= d.N * d.k) return;
    const int img = t / d.k, j = t - img * d.k;
    const long long o = (long long)img * ld + j;
    const int i = idx[o];
    float x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f;
    int ok = 0;
    if (i >= 0 && i < d.H * d.W * d.A) {
        const int pix = i / d.A, a = i - pix * d.A, y = pix / d.W, x = pix - y * d.W;
        const float* q = dl.p + (long long)img * dl.sN + (long long)y * dl.sH + (long long)x * dl.sW + 4 * a;
        // in fp64: pcx = dx w + cx cancels when a delta moves a far anchor back towards the origin, and the fp32 rounding of the anchor's
        // own coordinates (up to half an ulp of x stride) would then exceed every bound stated relative to |pcx| + pw.  2000 boxes per level.
        const double sx = (double)(x * d.stride), sy = (double)(y * d.stride);
        const double ax1 = (double)cell[4 * a] + sx, ay1 = (double)cell[4 * a + 1] + sy, ax2 = (double)cell[4 * a + 2] + sx,
                     ay2 = (double)cell[4 * a + 3] + sy;
        const double w = ax2 - ax1, h = ay2 - ay1, cx = ax1 + 0.5 * w, cy = ay1 + 0.5 * h;
        const double dx = (double)q[0] / (double)d.wx, dy = (double)q[1] / (double)d.wy;
        const double dw = fmin((double)q[2] / (double)d.ww, d.clamp), dh = fmin((double)q[3] / (double)d.wh, d.clamp);
        const double pcx = dx * w + cx, pcy = dy * h + cy, pw = exp(dw) * w, ph = exp(dh) * h;
        const float ih = image_hw[2 * img], iw = image_hw[2 * img + 1];
        x1 = fminf(fmaxf((float)(pcx - 0.5 * pw), 0.f), iw);
        y1 = fminf(fmaxf((float)(pcy - 0.5 * ph), 0.f), ih);
        x2 = fminf(fmaxf((float)(pcx + 0.5 * pw), 0.f), iw);
        y2 = fminf(fmaxf((float)(pcy + 0.5 * ph), 0.f), ih);
        ok = (x2 - x1 > d.min_size) && (y2 - y1 > d.min_size);
    }
    float* b = boxes + 4 * o;
    b[0] = x1; b[1] = y1; b[2] = x2; b[3] = y2;
    valid[o] = ok;
}

int afi_rpn_decode(afi_view_t deltas, int N, int H, int W, int A, const float* cell_anchors, int stride, const int* idx, int k, long long ld,
                   const float* image_hw, float wx, float wy, float ww, float wh, double scale_clamp, float min_size, float* boxes, int* valid,
                   void* stream) {
    if (!deltas.p || !cell_anchors || !idx || !image_hw || !boxes || !valid || N <= 0 || H <= 0 || W <= 0 || A <= 0 || stride <= 0 || k <= 0 ||
        ld < k)
        return AFI_ERR_BAD_ARG;
    if (A > RPN_MAX_A || (long long)H * W * A >= RPN_IDX_MASK || (long long)N * k > (1ll << 30)) return AFI_ERR_UNSUPPORTED;
    if (!(wx > 0.f) || !(wy > 0.f) || !(ww > 0.f) || !(wh > 0.f)) return AFI_ERR_BAD_ARG;
    const AfiView dl{(float*)deltas.p, deltas.sN, deltas.sH, deltas.sW};
    const RpnDecode d{N, H, W, A, k, stride, wx, wy, ww, wh, scale_clamp, min_size};
    hipLaunchKernelGGL(afi_rpn_decode_kernel, dim3((N * k + 255) / 256), dim3(256), 0, (hipStream_t)stream, dl, d, cell_anchors, idx, ld, image_hw,
                       boxes, valid);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}

// ------------------------------------------------------------------------------------------------ NMS
int afi_rpn_nms(const float* boxes, const int* valid, int N, int k, long long ld, float thresh, int* keep, void* stream) {
    if (N <= 0 || N > 65535 || k < 0 || ld < k) return AFI_ERR_BAD_ARG;
    if (k == 0) return AFI_OK;
    if (!boxes || !valid || !keep) return AFI_ERR_BAD_ARG;
    if (k > RPN_MAXK) return AFI_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(afi_nms_kernel<false>, dim3(N), dim3(1024), 0, (hipStream_t)stream, boxes, (const int*)nullptr, valid, k, ld, thresh,
                       keep);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}

// afi_rpn_nms_wide, lists of up to RPN_MAXK_WIDE boxes.  The bit matrix in the workspace: per image k rows of nw = ceil(k / 64) words,
// mask[i][w] bit j as in afi_nms_kernel.  Build: one block per 64 x 64 tile (column word w, row tile rt <= w) of the upper triangle,
// blockIdx.x = w (w + 1) / 2 + rt; a wave takes sixteen rows, a lane is a column, a wave's __ballot is the word.
__global__ __launch_bounds__(256) void afi_rpn_nms_build_kernel(const float* __restrict__ boxes, const int* __restrict__ valid, int k, long long ld,
                                                                float thresh, u64* __restrict__ mask_all) {
    const int img = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nw = (k + 63) >> 6, t = blockIdx.x;
    int w = (int)((sqrtf(8.f * (float)t + 1.f) - 1.f) * 0.5f);
    while ((w + 1) * (w + 2) / 2 <= t) ++w;
    while (w * (w + 1) / 2 > t) --w;
    const int rt = t - w * (w + 1) / 2;
    if (w >= nw || rt > w) return;                      // (never: the grid is nw (nw + 1) / 2 wide)
    const int j = 64 * w + lane;
    float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
    bool cok = false;
    if (j < k) {
        const float* q = boxes + 4 * ((long long)img * ld + j);
        c = make_float4(q[0], q[1], q[2], q[3]);
        cok = valid[(long long)img * ld + j] != 0;
    }
    u64* mask = mask_all + (long long)img * k * nw;
    const int i0 = 64 * rt + 16 * wave;
    for (int s = 0; s < 16; ++s) {
        const int i = i0 + s;
        if (i >= k) break;
        const float* q = boxes + 4 * ((long long)img * ld + i);
        const float4 r = make_float4(q[0], q[1], q[2], q[3]);
        const bool hit = cok && j > i && rpn_overlaps(r, c, thresh);
        const u64 word = __ballot(hit);
        if (lane == 0) mask[(long long)i * nw + w] = word;
    }
}

// One wave per image; lane w holds word w of the boxes suppressed so far.  Per chunk of 64 rows: the diagonal word resolved in registers
// (rpn_resolve_diag), then the kept rows' words OR-ed in -- sixteen rows' loads issued together (a row is nw <= 64 words: one coalesced read), rows
// of a group that were not kept are read and masked out, a group without a kept row is skipped.  Only words the build wrote are read: column
// words w > c of rows 64 c .. min(64 c + 63, k - 1), and the diagonal words.
__global__ __launch_bounds__(64) void afi_rpn_nms_sweep_kernel(const u64* __restrict__ mask_all, const int* __restrict__ valid, int k, long long ld,
                                                               int* __restrict__ keep) {
    const int img = blockIdx.x, lane = threadIdx.x;
    const int nw = (k + 63) >> 6;
    const u64* mask = mask_all + (long long)img * k * nw;
    u64 remv = 0;
    for (int c = 0; c < nw; ++c) {
        const int row = 64 * c + lane;
        const u64 diag = (row < k) ? mask[(long long)row * nw + c] : 0ull;
        const u64 V = __ballot(row < k && valid[(long long)img * ld + (row < k ? row : 0)] != 0);
        const u64 K = rpn_resolve_diag(rpn_readlane64(remv, c) | ~V, diag);      // an invalid box is neither kept nor suppresses anything
        if (row < k) keep[(long long)img * ld + row] = (int)((K >> lane) & 1ull);
        const bool mine = lane > c && lane < nw;
        u64 acc = 0;
        for (int g = 0; g < 64; g += 16) {
            if (!mine || !((K >> g) & 0xFFFFull)) continue;
            u64 v[16];
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                int r = 64 * c + g + s;
                r = r < k ? r : k - 1;                  // (a row past the list is never kept: its word is masked out below)
                v[s] = mask[(long long)r * nw + lane];
            }
#pragma unroll
            for (int s = 0; s < 16; ++s)
                if ((K >> (g + s)) & 1ull) acc |= v[s];
        }
        remv |= acc;
    }
}

long long afi_rpn_nms_wide_ws_floats(int N, int k) {
    if (N <= 0 || k < 0 || k > RPN_MAXK_WIDE) return -1;
    return 2ll * N * k * ((k + 63) / 64);
}

int afi_rpn_nms_wide(const float* boxes, const int* valid, int N, int k, long long ld, float thresh, int* keep, float* ws, long long ws_floats,
                     void* stream) {
    if (N <= 0 || N > 65535 || k < 0 || ld < k) return AFI_ERR_BAD_ARG;
    if (k == 0) return AFI_OK;
    if (!boxes || !valid || !keep) return AFI_ERR_BAD_ARG;
    if (k > RPN_MAXK_WIDE) return AFI_ERR_UNSUPPORTED;
    if (!ws || ws_floats < afi_rpn_nms_wide_ws_floats(N, k) || ((uintptr_t)ws & 7)) return AFI_ERR_WORKSPACE;
    const int nw = (k + 63) / 64;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(afi_rpn_nms_build_kernel, dim3(nw * (nw + 1) / 2, N), dim3(256), 0, st, boxes, valid, k, ld, thresh, (u64*)ws);
    hipLaunchKernelGGL(afi_rpn_nms_sweep_kernel, dim3(N), dim3(64), 0, st, (const u64*)ws, valid, k, ld, keep);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}

// ------------------------------------------------------------------------------------------------ merge
// boxes [N][Ktot][4], vals / keep [N][Ktot]: the levels side by side, level l in columns [off[l], off[l + 1]), each sorted by afi_rpn_topk.
// Ktot <= TOTAL < 65536 (positions are 16 bits).  The threads take a level's entries in chunks of 1024, one block scan per chunk: one chunk
// for a level of <= RPN_MAXK entries.
template <int TOTAL>
__global__ __launch_bounds__(1024) void afi_rpn_merge_kernel(const float* __restrict__ boxes, const float* __restrict__ vals,
                                                             const int* __restrict__ keep, const RpnLevels lv, int post_k,
                                                             float* __restrict__ ob, float* __restrict__ ol, int* __restrict__ counts) {
    __shared__ unsigned ckey[TOTAL];
    __shared__ unsigned short cpos[TOTAL];
    __shared__ int cnt[RPN_MAX_LEVELS];
    __shared__ int wtot[16];
    const int img = blockIdx.x, tid = threadIdx.x, Ktot = lv.off[lv.L];
    const long long row0 = (long long)img * Ktot;
    for (int l = 0; l < lv.L; ++l) {
        const int o = lv.off[l], kl = lv.off[l + 1] - o;
        int base = 0;
        for (int e0 = 0; e0 < kl; e0 += 1024) {
            const int e = e0 + tid;
            const int f = (e < kl) && keep[row0 + o + (e < kl ? e : 0)] != 0;
            int tot;
            const int inc = rpn_block_scan(f, wtot, &tot);
            if (f) {
                ckey[o + base + inc - 1] = rpn_key(vals[row0 + o + e]);
                cpos[o + base + inc - 1] = (unsigned short)(o + e);
            }
            base += tot;
        }
        if (tid == 0) cnt[l] = base;
    }
    __syncthreads();
    int total = 0;
    for (int l = 0; l < lv.L; ++l) total += cnt[l];
    for (int l = 0; l < lv.L; ++l) {
        for (int e = tid; e < cnt[l]; e += 1024) {
            const unsigned key = ckey[lv.off[l] + e];
            int rank = e;
            for (int b = 0; b < lv.L && rank < post_k; ++b) {
                if (b == l) continue;
                const unsigned* arr = ckey + lv.off[b];
                int lo = 0, hi = cnt[b];
                while (lo < hi) {                          // entries of level b in front: >= key for an earlier level, > key for a later one
                    const int mid = (lo + hi) >> 1;
                    const bool front = b < l ? arr[mid] >= key : arr[mid] > key;
                    if (front) lo = mid + 1; else hi = mid;
                }
                rank += lo;
            }
            if (rank < post_k) {
                const long long src = row0 + cpos[lv.off[l] + e], dst = (long long)img * post_k + rank;
                const float* q = boxes + 4 * src;
                float* p = ob + 4 * dst;
                p[0] = q[0]; p[1] = q[1]; p[2] = q[2]; p[3] = q[3];
                ol[dst] = vals[src];
            }
        }
    }
    const int c = total < post_k ? total : post_k;
    if (tid == 0) counts[img] = c;
    for (int r = c + tid; r < post_k; r += 1024) {
        const long long dst = (long long)img * post_k + r;
        float* p = ob + 4 * dst;
        p[0] = 0.f; p[1] = 0.f; p[2] = 0.f; p[3] = 0.f;
        ol[dst] = 0.f;
    }
}

// Levels of at most LEVEL_MAX entries, TOTAL over all levels (RPN_MAX_LEVELS levels of RPN_MAXK never exceed the narrow TOTAL).
template <int LEVEL_MAX, int TOTAL>
static int rpn_merge_launch(const float* boxes, const float* vals, const int* keep, int N, int L, const int* level_off, int post_k,
                            float* out_boxes, float* out_logits, int* counts, void* stream) {
    if (!boxes || !vals || !keep || !level_off || !out_boxes || !out_logits || !counts || N <= 0 || N > 65535 || L <= 0 || post_k <= 0)
        return AFI_ERR_BAD_ARG;
    if (L > RPN_MAX_LEVELS) return AFI_ERR_UNSUPPORTED;
    RpnLevels lv;
    lv.L = L;
    if (level_off[0] != 0) return AFI_ERR_BAD_ARG;
    for (int l = 0; l <= RPN_MAX_LEVELS; ++l) lv.off[l] = level_off[l < L ? l : L];
    for (int l = 0; l < L; ++l) {
        const int kl = level_off[l + 1] - level_off[l];
        if (kl < 0) return AFI_ERR_BAD_ARG;
        if (kl > LEVEL_MAX) return AFI_ERR_UNSUPPORTED;
    }
    if (level_off[L] <= 0) return AFI_ERR_BAD_ARG;
    if (level_off[L] > TOTAL) return AFI_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(afi_rpn_merge_kernel<TOTAL>, dim3(N), dim3(1024), 0, (hipStream_t)stream, boxes, vals, keep, lv, post_k, out_boxes,
                       out_logits, counts);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}

int afi_rpn_merge(const float* boxes, const float* vals, const int* keep, int N, int L, const int* level_off, int post_k, float* out_boxes,
                  float* out_logits, int* counts, void* stream) {
    return rpn_merge_launch<RPN_MAXK, RPN_MAX_LEVELS * RPN_MAXK>(boxes, vals, keep, N, L, level_off, post_k, out_boxes, out_logits, counts, stream);
}

int afi_rpn_merge_wide(const float* boxes, const float* vals, const int* keep, int N, int L, const int* level_off, int post_k, float* out_boxes,
                       float* out_logits, int* counts, void* stream) {
    return rpn_merge_launch<RPN_MAXK_WIDE, RPN_WIDE_TOTAL>(boxes, vals, keep, N, L, level_off, post_k, out_boxes, out_logits, counts, stream);
}
