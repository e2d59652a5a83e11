// What the selection stages of the RPN (rpn.hip), its training-side sampler (rpn_loss.hip) and the ROI heads' box branch (roi.hip) share: the
// block prefix sum, the radix select and its digit search, the overlap test and the diagonal resolve of the greedy NMS, and the NMS of a sorted
// list of <= 1024 boxes, with or without classes.
#pragma once
#include "afi_common.h"

#define RPN_MAXK 1024
#define RPN_MAXK_WIDE 4096                  // the "wide" selection of rpn.hip: 64 x 64, so the suppressed set is one 64-bit word per lane of a wave
#define RPN_WIDE_TOTAL (5 * RPN_MAXK_WIDE)  // entries of all levels of an image afi_rpn_merge_wide holds in LDS (keys 80 KiB + positions 40 KiB)

typedef unsigned long long u64;

// Inclusive prefix sum over the block (blockDim a multiple of 64, <= 1024); wtot: 16 ints of LDS.  Two barriers.
__device__ __forceinline__ int rpn_block_scan(int v, int* wtot, int* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    __syncthreads();
    if (lane == 63) wtot[w] = inc;
    __syncthreads();
    int base = 0, tot = 0;
    for (int i = 0; i < nw; ++i) {
        const int t = wtot[i];
        if (i < w) base += t;
        tot += t;
    }
    *total = tot;
    return inc + base;
}

// The digit d of a histogram (nbins a multiple of blockDim) that holds the need-th element counted from the top bin down, and the count of
// the bins above it: res[0] = d, res[1] = above.  1 <= need <= sum(hist).  Ends with a barrier; hist is left as it was.  (The radix select of
// afi_rpn_topk and of afi_rpn_sample.)
__device__ __forceinline__ void rpn_find_digit(const int* hist, int nbins, int need, int* wtot, int* res) {
    const int per = nbins / (int)blockDim.x, top = nbins - 1 - (int)threadIdx.x * per;
    int own = 0;
    for (int j = 0; j < per; ++j) own += hist[top - j];
    if (threadIdx.x == 0) { res[0] = 0; res[1] = 0; }
    int total;
    const int inc = rpn_block_scan(own, wtot, &total);
    int cum = inc - own;
    if (cum < need && need <= inc) {
        for (int j = 0; j < per; ++j) {
            const int c = hist[top - j];
            if (cum + c >= need) { res[0] = top - j; res[1] = cum; break; }
            cum += c;
        }
    }
    __syncthreads();
}

// The radix select over 64-bit words (a 32-bit key above idx_bits index bits: distinct words), by a block of 1024 threads: the cut below which
// none of the `need` largest words of the members lies.  word(i, &c) says whether element i < count takes part and writes its word; `group` is
// the number of members.  Digits of 11, 11, 10 key bits, then 11, 11 index bits; the passes stop as soon as the open digit group is taken whole
// (need == group) or nothing is wanted.  Afterwards the members with (word >> shift) >= prefix are the min(need, group) largest (for need == 0
// the cut is open: the caller takes none).  hist: 2048 ints of LDS, wtot: 16, res: 2.  Every pass ends with a barrier.
struct RpnCut { int shift; u64 prefix; };

template <class Word>
__device__ __forceinline__ RpnCut rpn_radix_select(Word word, int count, int group, int need, int idx_bits, int* hist, int* wtot, int* res) {
    const int tid = threadIdx.x;
    int shift = 32 + idx_bits;
    u64 prefix = 0;
    const int widths[5] = {11, 11, 10, 11, 11};
    for (int p = 0; p < 5 && need > 0 && need < group; ++p) {
        const int bits = widths[p], nb = 1 << bits;
        shift -= bits;
        for (int i = tid; i < nb; i += 1024) hist[i] = 0;
        __syncthreads();
        for (int i = tid; i < count; i += 1024) {
            u64 c;
            if (!word(i, &c)) continue;
            if ((c >> (shift + bits)) == prefix) atomicAdd(&hist[(int)(c >> shift) & (nb - 1)], 1);
        }
        __syncthreads();
        rpn_find_digit(hist, nb, need, wtot, res);
        need -= res[1];
        group = hist[res[0]];
        prefix = (prefix << bits) | (u64)res[0];
        __syncthreads();
    }
    return RpnCut{shift, prefix};
}

// ------------------------------------------------------------------------------------------------ NMS
// The overlap test of every NMS here: box c (later in the list) against box r, inter / (rarea + carea - inter) > thresh, each operation
// rounded to fp32 -- no fused multiply-add: the pragma is part of the rule.  (carea does not depend on r: the compiler hoists it out of a loop
// over rows.)
__device__ __forceinline__ bool rpn_overlaps(const float4 r, const float4 c, float thresh) {
#pragma clang fp contract(off)
    const float iw = fmaxf(fminf(r.z, c.z) - fmaxf(r.x, c.x), 0.f), ih = fmaxf(fminf(r.w, c.w) - fmaxf(r.y, c.y), 0.f);
    const float inter = iw * ih, rarea = (r.z - r.x) * (r.w - r.y), carea = (c.z - c.x) * (c.w - c.y);
    return inter / (rarea + carea - inter) > thresh;
}

__device__ __forceinline__ u64 rpn_readlane64(u64 v, int lane) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, lane);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), lane);
    return ((u64)hi << 32) | lo;
}

// The greedy pass over 64 consecutive boxes of a sorted list, by one wave: bit b of R says box b is out already (suppressed by an earlier
// chunk, or invalid), lane b's diag has bit j set where box b suppresses box j > b of the chunk.  Returns the kept boxes as one word.
__device__ __forceinline__ u64 rpn_resolve_diag(u64 R, u64 diag) {
    u64 K = 0;
#pragma unroll
    for (int b = 0; b < 64; ++b) {
        if (!((R >> b) & 1ull)) {
            K |= 1ull << b;
            R |= rpn_readlane64(diag, b);
        }
    }
    return K;
}

// One block (sixteen waves) per image.  mask[i][w] bit j: box 64 w + j (later than i in the list) overlaps box i by more than thresh.
// CLS: a pair suppresses only when its classes are equal (afi_roi_nms): one more LDS array and one more term of the test; !CLS is afi_rpn_nms as it was.
template <bool CLS>
__global__ __launch_bounds__(1024) void afi_nms_kernel(const float* __restrict__ boxes, const int* __restrict__ cls, const int* __restrict__ valid,
                                                       int k, long long ld, float thresh, int* __restrict__ keep) {
    __shared__ u64 mask[RPN_MAXK * 16];
    __shared__ float4 bx[RPN_MAXK];
    __shared__ int vd[RPN_MAXK];
    __shared__ int cl[CLS ? RPN_MAXK : 1];
    const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nw = (k + 63) >> 6;
    {
        float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
        int v = 0;
        if (tid < k) {
            const float* q = boxes + 4 * ((long long)img * ld + tid);
            b = make_float4(q[0], q[1], q[2], q[3]);
            v = valid[(long long)img * ld + tid] != 0;
        }
        bx[tid] = b;
        vd[tid] = v;
        if (CLS) cl[tid] = tid < k ? cls[(long long)img * ld + tid] : -1;
    }
    __syncthreads();
    for (int w = 0; w < nw; ++w) {
        const int j = 64 * w + lane;
        const float4 c = bx[j];
        const bool cok = j < k && vd[j];
        const int ccls = CLS ? cl[j] : 0;
        const int rows = 64 * (w + 1) < k ? 64 * (w + 1) : k;
        for (int i = wave; i < rows; i += 16) {
            const float4 r = bx[i];
            const bool hit = cok && j > i && (!CLS || cl[i] == ccls) && rpn_overlaps(r, c, thresh);
            const u64 word = __ballot(hit);
            if (lane == 0) mask[i * 16 + w] = word;
        }
    }
    __syncthreads();
    if (wave != 0) return;
    u64 remv = 0;                                       // lane w < 16: word w of the boxes suppressed so far
    const int wsel = lane & 15, sub = lane >> 4;
    for (int c = 0; c < nw; ++c) {
        const int row = 64 * c + lane;
        const u64 diag = (row < k) ? mask[row * 16 + c] : 0ull;
        const u64 V = __ballot(row < k && vd[row]);
        const u64 K = rpn_resolve_diag(rpn_readlane64(remv, c) | ~V, diag);      // an invalid box is neither kept nor suppresses anything
        if (row < k) keep[(long long)img * ld + row] = (int)((K >> lane) & 1ull);
        // OR the kept rows' words into remv: lane = (word wsel, rows sub, sub + 4, ...)
        u64 acc = 0;
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const int b = sub + 4 * t;
            if (wsel > c && wsel < nw && ((K >> b) & 1ull)) acc |= mask[(64 * c + b) * 16 + wsel];
        }
        acc |= __shfl_xor(acc, 16, 64);
        acc |= __shfl_xor(acc, 32, 64);
        remv |= acc;                                    // lanes >= 16 hold copies of words lane & 15: never read
    }
}
