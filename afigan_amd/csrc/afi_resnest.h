// What resnest.hip (the frozen forward) and resnest_train.hip (the backward) share: the argument checks, the float4 view load and the
// chunk geometry of the pooled-sum passes (the backward's dot products run on the forward's chunks).
#pragma once
#include <stdint.h>

#include "../../include/afigan_hip.h"
#include "afi_common.h"

#define RS_GAP_BYTES 65536      // bytes of one split a gap block reads per chunk (chunk pixels = RS_GAP_BYTES / (4 C), at least a block's slots)
#define RS_MAX_C 1024           // split width limit of the gap pass (C / 4 float4 lanes <= 256 threads)

static inline unsigned grid_of(long long work, long long cap) {
    long long b = (work + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

static inline bool view_ok(const afi_view_t& v) {
    return v.p && !((uintptr_t)v.p & 15) && !(v.sN & 3) && !(v.sH & 3) && !(v.sW & 3);
}

__device__ __forceinline__ f32x4 ld4(const AfiView& v, int n, int y, int x, int c) {
    return *(const f32x4*)(v.p + n * v.sN + y * v.sH + x * v.sW + c);
}

// The chunking of the pooled-sum pass, shared by its launcher, the attention pass and the workspace query: a 256-thread block holds
// 256 / (C / 4) pixel slots x C / 4 float4 lanes and sums one chunk of about RS_GAP_BYTES per split.
static inline int gap_slots(int C) { return 256 / (C >> 2); }
static inline int gap_chunk_pix(int C) {
    const int p = RS_GAP_BYTES / (4 * C), s = gap_slots(C);
    return p > s ? p : s;
}
static inline int gap_chunks(int H, int W, int C) { return (int)(((long long)H * W + gap_chunk_pix(C) - 1) / gap_chunk_pix(C)); }
