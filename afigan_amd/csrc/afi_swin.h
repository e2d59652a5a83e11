// What the Swin kernels of swin.hip (forward) and swin_train.hip (backward) share: the constants, the launch helpers and the wave reduction.
// The index arithmetic of a window token (roll, pad, partition, shift region) is swin_window_token below: the forward kernel states it inline
// (its body is unchanged); the backward kernels call it.
#pragma once
#include "afi_common.h"

#define SW_EMBED_MAXC 256       // patch-embed channels (4 per lane)
#define SW_LN_MAXV 12           // float4s per lane of a LayerNorm token: 12 * 4 * 64 = 3072 channels (4C of Swin-L's last merge)
#define SW_HEAD_DIM 32
#define SW_LDS_LD 36            // LDS row stride of the q / k / v tiles: 36 j + k (k < 4) covers 64 banks with 16 rows, and rows stay 16-byte aligned

typedef float f32x4_mfma __attribute__((ext_vector_type(4)));

static inline unsigned grid_of(long long work, long long per_block, long long cap) {
    long long b = (work + per_block - 1) / per_block;
    return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

static inline bool view_ok(const afi_view_t& v) {
    return v.p && !((uintptr_t)v.p & 15) && !(v.sN & 3) && !(v.sH & 3) && !(v.sW & 3);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Window token t (< WS^2) of the window at (wy0, wx0) of the rolled, padded Hp x Wp map: its un-rolled pixel (py, px) -- inside Hp x Wp, a
// padded token where py >= H or px >= W -- and its shift region (0 without a shift): afi_swin_attn_kernel's arithmetic.
__device__ __forceinline__ void swin_window_token(int t, int WS, int wy0, int wx0, int Hp, int Wp, int shift, int& py, int& px, int& reg) {
    const int ry = wy0 + t / WS, rx = wx0 + t % WS;
    py = (ry + shift) % Hp; px = (rx + shift) % Wp;
    reg = shift ? 3 * (ry < Hp - WS ? 0 : (ry < Hp - shift ? 1 : 2)) + (rx < Wp - WS ? 0 : (rx < Wp - shift ? 1 : 2)) : 0;
}
