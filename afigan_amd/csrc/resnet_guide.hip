// The two kernels of the frozen ResNet-FPN guide (afigan_amd/resnet_guide.py) that no other launcher covers; every other conv of the
// guide runs on the pixel GEMM / Winograd launchers of igemm.hip and winograd.hip.
//   afi_resnet_stem_fwd  detectron2's BasicStem: Conv2d(3, 64, 7, stride 2, pad 3) with the FrozenBN affine folded into weight and bias,
//                        ReLU, then max_pool2d(3, stride 2, pad 1) -- in ONE kernel.  A block owns an 8 x 8 tile of POOLED pixels and 32
//                        of the 64 channels: it computes the 17 x 17 conv outputs under that tile (the tile plus a one-pixel halo) into
//                        LDS and pools them there, so the 64 x H/2 x W/2 conv map is never written.
//   afi_nearest_nhwc     nearest resampling by an integer ratio on the pixel-major layout: the FPN's x2 top-down up-sampling (its
//                        result is the `add=` operand of the lateral 1x1 conv) and LastLevelMaxPool's stride-2 subsampling (p6).
#include "../../include/afigan_hip.h"
#include "afi_common.h"

#define STEM_TP 8                       // pooled tile edge
#define STEM_TC (2 * STEM_TP + 1)       // conv tile edge (the pooled tile's windows: 2 * 8 + 1 rows / columns)
#define STEM_NPOS (STEM_TC * STEM_TC)   // 289 conv positions
#define STEM_TI (2 * (STEM_TC - 1) + 7) // input tile edge (39)
#define STEM_TIW 40                     // its LDS row pitch
#define STEM_CB 32                      // output channels per block
#define STEM_CS 33                      // LDS pitch of one conv position (32 channels + 1: conflict-free stores across positions)
#define STEM_PPL 5                      // conv positions per lane: 64 lanes x 5 = 320 >= 289
#define STEM_K 147                      // 3 x 7 x 7 taps

// x: dense NCHW [N][3][H][W] fp32; w: dense [64][3][7][7] (OIHW, the affine folded in); bias[64]; out: dense [N][Ho][Wo][64].
// Thread t: channel group g = t / 64 (8 channels, uniform per wave: the weight reads are broadcasts), lane l = t % 64 owns conv positions
// l + 64 j.  Zero padding for the conv (outside the image), -inf for the pool (conv positions outside the conv map).
__global__ __launch_bounds__(256) void afi_resnet_stem_kernel(const float* __restrict__ x, int H, int W, const float* __restrict__ w,
                                                              const float* __restrict__ bias, int Hc, int Wc, int Ho, int Wo,
                                                              float* __restrict__ out) {
    __shared__ float xs[3 * STEM_TI * STEM_TIW];
    __shared__ float ws[STEM_K * STEM_CB];
    __shared__ float cs[STEM_NPOS * STEM_CS];
    const int tid = threadIdx.x;
    const int n = blockIdx.z >> 1, half = blockIdx.z & 1;
    const int oy0 = blockIdx.y * STEM_TP, ox0 = blockIdx.x * STEM_TP;
    const int cy0 = 2 * oy0 - 1, cx0 = 2 * ox0 - 1;             // conv tile origin (the pool's top / left pad row is row -1)
    const int iy0 = 2 * cy0 - 3, ix0 = 2 * cx0 - 3;             // input tile origin
    const float* xn = x + (long long)n * 3 * H * W;
    for (int i = tid; i < 3 * STEM_TI * STEM_TI; i += 256) {
        const int c = i / (STEM_TI * STEM_TI), r = i % (STEM_TI * STEM_TI);
        const int ly = r / STEM_TI, lx = r % STEM_TI;
        const int gy = iy0 + ly, gx = ix0 + lx;
        float v = 0.f;
        if ((unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W) v = xn[(long long)c * H * W + (long long)gy * W + gx];
        xs[(c * STEM_TI + ly) * STEM_TIW + lx] = v;
    }
    const float* wh = w + (long long)half * STEM_CB * STEM_K;
    for (int i = tid; i < STEM_CB * STEM_K; i += 256) {
        const int co = i / STEM_K, k = i % STEM_K;
        ws[k * STEM_CB + co] = wh[i];
    }
    __syncthreads();

    const int g = tid >> 6, lane = tid & 63;
    int base[STEM_PPL];
#pragma unroll
    for (int j = 0; j < STEM_PPL; ++j) {
        const int pos = lane + 64 * j;
        const int p = pos < STEM_NPOS ? pos : 0;                 // (slots past the tile compute position 0 again and are not stored)
        base[j] = 2 * (p / STEM_TC) * STEM_TIW + 2 * (p % STEM_TC);
    }
    f32x4 acc[STEM_PPL][2];
#pragma unroll
    for (int j = 0; j < STEM_PPL; ++j) acc[j][0] = acc[j][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < 3; ++c) {
        const float* xc = xs + c * STEM_TI * STEM_TIW;
        const float* wc = ws + c * 49 * STEM_CB + g * 8;
#pragma unroll 1
        for (int ky = 0; ky < 7; ++ky) {
#pragma unroll
            for (int kx = 0; kx < 7; ++kx) {
                const f32x4 wa = *(const f32x4*)(wc + (ky * 7 + kx) * STEM_CB);
                const f32x4 wb = *(const f32x4*)(wc + (ky * 7 + kx) * STEM_CB + 4);
#pragma unroll
                for (int j = 0; j < STEM_PPL; ++j) {
                    const float v = xc[base[j] + ky * STEM_TIW + kx];
                    acc[j][0] += v * wa;
                    acc[j][1] += v * wb;
                }
            }
        }
    }
    const float* bh = bias + half * STEM_CB + g * 8;
#pragma unroll
    for (int j = 0; j < STEM_PPL; ++j) {
        const int pos = lane + 64 * j;
        if (pos >= STEM_NPOS) continue;
        const int cy = cy0 + pos / STEM_TC, cx = cx0 + pos % STEM_TC;
        const bool inside = (unsigned)cy < (unsigned)Hc && (unsigned)cx < (unsigned)Wc;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const float v = fmaxf(acc[j][q >> 2][q & 3] + bh[q], 0.f);
            cs[pos * STEM_CS + g * 8 + q] = inside ? v : -INFINITY;
        }
    }
    __syncthreads();

    const int c = tid & 31;
    for (int p = tid >> 5; p < STEM_TP * STEM_TP; p += 8) {
        const int py = p / STEM_TP, px = p % STEM_TP;
        const int oy = oy0 + py, ox = ox0 + px;
        if (oy >= Ho || ox >= Wo) continue;
        float m = -INFINITY;
#pragma unroll
        for (int t = 0; t < 9; ++t) m = fmaxf(m, cs[((2 * py + t / 3) * STEM_TC + 2 * px + t % 3) * STEM_CS + c]);
        out[(((long long)n * Ho + oy) * Wo + ox) * 64 + half * STEM_CB + c] = m;
    }
}

int afi_resnet_stem_fwd(const float* x, int N, int H, int W, const float* w, const float* bias, float* out, void* stream) {
    if (!x || !w || !bias || !out || N <= 0 || H <= 0 || W <= 0 || N > 32767) return AFI_ERR_BAD_ARG;
    const int Hc = (H - 1) / 2 + 1, Wc = (W - 1) / 2 + 1;       // Conv2d(7, 2, 3)
    const int Ho = (Hc - 1) / 2 + 1, Wo = (Wc - 1) / 2 + 1;     // max_pool2d(3, 2, 1)
    const dim3 grid((Wo + STEM_TP - 1) / STEM_TP, (Ho + STEM_TP - 1) / STEM_TP, 2 * N);
    if (grid.y > 65535) return AFI_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(afi_resnet_stem_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, H, W, w, bias, Hc, Wc, Ho, Wo, out);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}

// out[n][oy][ox][c] = x[n][oy * down / up][ox * down / up][c]; one thread = one pixel x 4 channels
__global__ void afi_nearest_nhwc_kernel(const AfiView x, int N, int Ho, int Wo, int C, int up, int down, float* __restrict__ out) {
    const int C4 = C >> 2;
    const long long total = (long long)N * Ho * Wo * C4;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C4) * 4; long long r = i / C4;
        const int ox = (int)(r % Wo); r /= Wo; const int oy = (int)(r % Ho); const int n = (int)(r / Ho);
        const int sy = (int)((long long)oy * down / up), sx = (int)((long long)ox * down / up);
        *(f32x4*)(out + i * 4) = *(const f32x4*)(x.p + n * x.sN + sy * x.sH + sx * x.sW + c);
    }
}

int afi_nearest_nhwc(afi_view_t x, int N, int H, int W, int C, int up, int down, float* out, void* stream) {
    if (!x.p || !out || N <= 0 || H <= 0 || W <= 0 || C <= 0 || up < 1 || down < 1 || up > 64 || down > 64) return AFI_ERR_BAD_ARG;
    if ((C & 3) || ((uintptr_t)x.p & 15) || ((uintptr_t)out & 15) || (x.sN & 3) || (x.sH & 3) || (x.sW & 3)) return AFI_ERR_UNSUPPORTED;
    const long long Ho = ((long long)H * up + down - 1) / down, Wo = ((long long)W * up + down - 1) / down;
    const long long n4 = N * Ho * Wo * (C >> 2);
    long long blocks = (n4 + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    const AfiView v = {(float*)x.p, x.sN, x.sH, x.sW};
    hipLaunchKernelGGL(afi_nearest_nhwc_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, v, N, (int)Ho, (int)Wo, C, up, down, out);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}
