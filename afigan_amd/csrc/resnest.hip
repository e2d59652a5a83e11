// The kernels of the frozen ResNeSt bottom-up (afigan_amd/resnest_backbone.py) that no other launcher covers; its 1x1 convs run on
// afi_conv1x1_fwd and its 3x3 convs (the deep stem's second and third, and each radix group of a split-attention conv) on
// afi_conv3x3_fwd / afi_conv3x3_wino_infer.
//   afi_resnest_stem_fwd        the deep stem's first conv: Conv2d(3, Cout, 3, stride 2, pad 1) + folded norm + ReLU, reading the NCHW
//                               batch (Cin = 3 is not a multiple of 4, so no pixel-major conv can take it) and writing pixel-major.
//   afi_resnest_pool_nhwc       pixel-major pooling: max 3/2/1 (the stem), avg 3/2/1 counting the padding (AVD), avg 2/2 ceil mode not
//                               counting it (the avg_down shortcut).
//   afi_resnest_splat_gap       split attention, pass 1: per-chunk partial sums over the pixels of split0 + split1.
//   afi_resnest_splat_attn      pass 2, one block per image: the partials reduced in a fixed order, / (H*W), fc1 (+ folded bn1) + ReLU,
//                               fc2 + bias, the softmax over each radix pair.
//   afi_resnest_splat_combine   pass 3: a0 * split0 + a1 * split1, optionally with the AVD 3/2/1 average pool fused in.
// No atomics anywhere: every sum has one fixed order, so a forward is bit-identical from run to run and under hipGraph replay.
#include "afi_resnest.h"

#define RS_STEM_MAXC 128        // stem output channels held in LDS

// ------------------------------------------------------------------------------------------------ deep stem, first conv
// x dense NCHW [N][3][H][W]; w dense [Cout][3][3][3] in (O, kh, kw, I) order; out dense [N][Ho][Wo][Cout].  One thread = one output pixel x
// 4 channels (index pixel-major, so a wave's stores are contiguous); the 27 x Cout weights sit in LDS as [tap][Cout].
__global__ __launch_bounds__(256) void afi_resnest_stem_kernel(const float* __restrict__ x, int N, int H, int W, const float* __restrict__ w,
                                                               const float* __restrict__ bias, int Cout, int Ho, int Wo, float* __restrict__ out) {
    __shared__ f32x4 ws4[27 * RS_STEM_MAXC / 4];
    float* ws = (float*)ws4;
    for (int i = threadIdx.x; i < 27 * Cout; i += 256) ws[(i % 27) * Cout + i / 27] = w[i];
    __syncthreads();
    const int C4 = Cout >> 2;
    const long long total = (long long)N * Ho * Wo * C4;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % C4) * 4; long long r = i / C4;
        const int ox = (int)(r % Wo); r /= Wo; const int oy = (int)(r % Ho); const int n = (int)(r / Ho);
        const float* xn = x + (long long)n * 3 * H * W;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = 2 * oy - 1 + ky;
            if ((unsigned)iy >= (unsigned)H) continue;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = 2 * ox - 1 + kx;
                if ((unsigned)ix >= (unsigned)W) continue;
#pragma unroll
                for (int ci = 0; ci < 3; ++ci) {
                    const float v = xn[(long long)ci * H * W + (long long)iy * W + ix];
                    acc += v * *(const f32x4*)(ws + ((ky * 3 + kx) * 3 + ci) * Cout + c);
                }
            }
        }
        f32x4 o;
        o.x = fmaxf(acc.x + bias[c], 0.f);
        o.y = fmaxf(acc.y + bias[c + 1], 0.f);
        o.z = fmaxf(acc.z + bias[c + 2], 0.f);
        o.w = fmaxf(acc.w + bias[c + 3], 0.f);
        *(f32x4*)(out + i * 4) = o;
    }
}

int afi_resnest_stem_fwd(const float* x, int N, int H, int W, const float* w, const float* bias, int Cout, float* out, void* stream) {
    if (!x || !w || !bias || !out || N <= 0 || H <= 0 || W <= 0 || Cout <= 0) return AFI_ERR_BAD_ARG;
    if ((Cout & 3) || Cout > RS_STEM_MAXC || ((uintptr_t)out & 15)) return AFI_ERR_UNSUPPORTED;
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const long long total = (long long)N * Ho * Wo * (Cout >> 2);
    hipLaunchKernelGGL(afi_resnest_stem_kernel, dim3(grid_of(total, 4096)), dim3(256), 0, (hipStream_t)stream, x, N, H, W, w, bias, Cout, Ho,
                       Wo, out);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}

// ------------------------------------------------------------------------------------------------ pixel-major pooling
__global__ __launch_bounds__(256) void afi_resnest_pool_kernel(const AfiView x, int N, int H, int W, int C, int mode, int Ho, int Wo,
                                                              float* __restrict__ out) {
    const int C4 = C >> 2;
    const long long total = (long long)N * Ho * Wo * C4;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % C4) * 4; long long r = i / C4;
        const int ox = (int)(r % Wo); r /= Wo; const int oy = (int)(r % Ho); const int n = (int)(r / Ho);
        f32x4 o;
        if (mode == AFI_POOL_AVG2S2_CEIL) {                      // window [2oy, 2oy+2) x [2ox, 2ox+2) clipped to the map; divisor = pixels covered
            const int y0 = 2 * oy, x0 = 2 * ox, y1 = min(y0 + 2, H), x1 = min(x0 + 2, W);
            f32x4 s = {0.f, 0.f, 0.f, 0.f};
            for (int y = y0; y < y1; ++y)
                for (int xx = x0; xx < x1; ++xx) s += ld4(x, n, y, xx, c);
            o = s / (float)((y1 - y0) * (x1 - x0));
        } else {                                                 // window [2oy-1, 2oy+2) x [2ox-1, 2ox+2), padding -inf (max) / 0 (avg)
            const bool mx = mode == AFI_POOL_MAX3S2P1;
            f32x4 s = mx ? f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY} : f32x4{0.f, 0.f, 0.f, 0.f};
            for (int ky = 0; ky < 3; ++ky) {
                const int y = 2 * oy - 1 + ky;
                if ((unsigned)y >= (unsigned)H) continue;
                for (int kx = 0; kx < 3; ++kx) {
                    const int xx = 2 * ox - 1 + kx;
                    if ((unsigned)xx >= (unsigned)W) continue;
                    const f32x4 v = ld4(x, n, y, xx, c);
                    if (mx) {
                        s.x = fmaxf(s.x, v.x); s.y = fmaxf(s.y, v.y); s.z = fmaxf(s.z, v.z); s.w = fmaxf(s.w, v.w);
                    } else {
                        s += v;
                    }
                }
            }
            o = mx ? s : s / 9.f;
        }
        *(f32x4*)(out + i * 4) = o;
    }
}

int afi_resnest_pool_nhwc(afi_view_t x, int N, int H, int W, int C, int mode, float* out, void* stream) {
    if (!x.p || !out || N <= 0 || H <= 0 || W <= 0 || C <= 0) return AFI_ERR_BAD_ARG;
    if (mode != AFI_POOL_MAX3S2P1 && mode != AFI_POOL_AVG3S2P1 && mode != AFI_POOL_AVG2S2_CEIL) return AFI_ERR_BAD_ARG;
    if ((C & 3) || !view_ok(x) || ((uintptr_t)out & 15)) return AFI_ERR_UNSUPPORTED;
    const int Ho = mode == AFI_POOL_AVG2S2_CEIL ? (H + 1) / 2 : (H - 1) / 2 + 1;
    const int Wo = mode == AFI_POOL_AVG2S2_CEIL ? (W + 1) / 2 : (W - 1) / 2 + 1;
    const AfiView v = {x.p, x.sN, x.sH, x.sW};
    hipLaunchKernelGGL(afi_resnest_pool_kernel, dim3(grid_of((long long)N * Ho * Wo * (C >> 2), 8192)), dim3(256), 0, (hipStream_t)stream, v,
                       N, H, W, C, mode, Ho, Wo, out);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}

// ------------------------------------------------------------------------------------------------ split attention (radix 2, cardinality 1)
// (the chunk geometry gap_slots / gap_chunk_pix / gap_chunks: afi_resnest.h)
long long afi_resnest_splat_ws_floats(int N, int H, int W, int C) {
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || (C & 3) || C > RS_MAX_C) return 0;
    return (long long)N * gap_chunks(H, W, C) * C;
}

// part[n][k][c] = sum over pixels p of chunk k (ascending, by slot) of s0[n][p][c] + s1[n][p][c]; grid (chunks, N)
__global__ __launch_bounds__(256) void afi_resnest_splat_gap_kernel(const AfiView s0, const AfiView s1, int H, int W, int C, int chunk_pix,
                                                                   float* __restrict__ part) {
    __shared__ f32x4 red[256];
    const int C4 = C >> 2, slots = 256 / C4;
    const int tid = threadIdx.x, slot = tid / C4, c = (tid % C4) * 4;
    const int k = blockIdx.x, n = blockIdx.y;
    const long long HW = (long long)H * W;
    const long long p0 = (long long)k * chunk_pix, p1 = min(p0 + chunk_pix, HW);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (slot < slots) {
        for (long long p = p0 + slot; p < p1; p += slots) {
            const int y = (int)(p / W), x = (int)(p % W);
            acc += ld4(s0, n, y, x, c) + ld4(s1, n, y, x, c);
        }
    }
    red[tid] = acc;
    __syncthreads();
    if (tid < C4) {
        f32x4 s = red[tid];
        for (int j = 1; j < slots; ++j) s += red[j * C4 + tid];
        *(f32x4*)(part + ((long long)n * gridDim.x + k) * C + c) = s;
    }
}

int afi_resnest_splat_gap(afi_view_t s0, afi_view_t s1, int N, int H, int W, int C, float* part, long long part_floats, void* stream) {
    if (!s0.p || !s1.p || !part || N <= 0 || H <= 0 || W <= 0 || C <= 0) return AFI_ERR_BAD_ARG;
    if ((C & 3) || C > RS_MAX_C || !view_ok(s0) || !view_ok(s1) || ((uintptr_t)part & 15) || N > 65535) return AFI_ERR_UNSUPPORTED;
    if (part_floats < afi_resnest_splat_ws_floats(N, H, W, C)) return AFI_ERR_WORKSPACE;
    const AfiView v0 = {s0.p, s0.sN, s0.sH, s0.sW}, v1 = {s1.p, s1.sN, s1.sH, s1.sW};
    hipLaunchKernelGGL(afi_resnest_splat_gap_kernel, dim3(gap_chunks(H, W, C), N), dim3(256), 0, (hipStream_t)stream, v0, v1, H, W, C,
                       gap_chunk_pix(C), part);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// One block of RS_ATTN_THREADS per image (the pass is latency-bound: its work is spread over 16 waves).  LDS: the chunk-sum slots, gap[C],
// h[I], z[2C].  The partials are summed as float4 lanes by 1024 / (C / 4) slots, each over chunks slot, slot + slots, ..., then the slots in
// order; the dot products take 4 rows per wave at a time (float4 per lane, one butterfly reduction per row).  Every order is fixed.
#define RS_ATTN_THREADS 1024
__device__ __forceinline__ void dot4rows(const float* __restrict__ w, int K, int r0, const float* v, int lane, float d[4]) {
#pragma unroll
    for (int r = 0; r < 4; ++r) d[r] = 0.f;
    for (int k = lane * 4; k < K; k += 256) {
        const f32x4 g = *(const f32x4*)(v + k);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const f32x4 a = *(const f32x4*)(w + (long long)(r0 + r) * K + k);
            d[r] += a.x * g.x + a.y * g.y + a.z * g.z + a.w * g.w;
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) d[r] = wave_sum(d[r]);
}

__global__ __launch_bounds__(RS_ATTN_THREADS) void afi_resnest_splat_attn_kernel(const float* __restrict__ part, int nchunk, int C, int I,
                                                                                float hw, const float* __restrict__ w1,
                                                                                const float* __restrict__ b1, const float* __restrict__ w2,
                                                                                const float* __restrict__ b2, float* __restrict__ att,
                                                                                float* __restrict__ g_keep, float* __restrict__ h_keep) {
    __shared__ f32x4 red[RS_ATTN_THREADS];
    extern __shared__ f32x4 sm4[];
    float* gap = (float*)sm4;
    float* h = gap + C;
    float* z = h + I;
    const int n = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int C4 = C >> 2, slots = RS_ATTN_THREADS / C4, slot = tid / C4, c = (tid % C4) * 4;
    const float* pn = part + (long long)n * nchunk * C;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (slot < slots)
        for (int k = slot; k < nchunk; k += slots) acc += *(const f32x4*)(pn + (long long)k * C + c);
    red[tid] = acc;
    __syncthreads();
    if (tid < C4) {
        f32x4 s = red[tid];
        for (int j = 1; j < slots; ++j) s += red[j * C4 + tid];
        *(f32x4*)(gap + c) = s / hw;
        if (g_keep) *(f32x4*)(g_keep + (long long)n * C + c) = s / hw;
    }
    __syncthreads();
    for (int j0 = wave * 4; j0 < I; j0 += RS_ATTN_THREADS / 16) {          // fc1 with bn1 folded, ReLU
        float d[4];
        dot4rows(w1, C, j0, gap, lane, d);
        if (lane < 4) {
            const float v = fmaxf((lane == 0 ? d[0] : lane == 1 ? d[1] : lane == 2 ? d[2] : d[3]) + b1[j0 + lane], 0.f);
            h[j0 + lane] = v;
            if (h_keep) h_keep[(long long)n * I + j0 + lane] = v;
        }
    }
    __syncthreads();
    for (int o0 = wave * 4; o0 < 2 * C; o0 += RS_ATTN_THREADS / 16) {      // fc2 + bias
        float d[4];
        dot4rows(w2, I, o0, h, lane, d);
        if (lane < 4) z[o0 + lane] = (lane == 0 ? d[0] : lane == 1 ? d[1] : lane == 2 ? d[2] : d[3]) + b2[o0 + lane];
    }
    __syncthreads();
    for (int i = tid; i < C; i += RS_ATTN_THREADS) {             // rSoftMax: softmax over (z[i], z[C + i])
        const float z0 = z[i], z1 = z[C + i], m = fmaxf(z0, z1);
        const float e0 = expf(z0 - m), e1 = expf(z1 - m), s = e0 + e1;
        att[(long long)n * 2 * C + i] = e0 / s;
        att[(long long)n * 2 * C + C + i] = e1 / s;
    }
}

static int splat_attn_launch(const float* part, int N, int H, int W, int C, int I, const float* w1, const float* b1, const float* w2,
                             const float* b2, float* att, float* g_keep, float* h_keep, void* stream) {
    if (!part || !w1 || !b1 || !w2 || !b2 || !att || N <= 0 || H <= 0 || W <= 0 || C <= 0 || I <= 0) return AFI_ERR_BAD_ARG;
    if ((C & 3) || (I & 3) || C > RS_MAX_C || I > 4 * RS_MAX_C || ((uintptr_t)w1 & 15) || ((uintptr_t)w2 & 15)) return AFI_ERR_UNSUPPORTED;
    const size_t lds = (size_t)(3 * C + I) * sizeof(float);
    hipLaunchKernelGGL(afi_resnest_splat_attn_kernel, dim3(N), dim3(RS_ATTN_THREADS), lds, (hipStream_t)stream, part, gap_chunks(H, W, C), C, I,
                       (float)((double)H * W), w1, b1, w2, b2, att, g_keep, h_keep);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}

int afi_resnest_splat_attn(const float* part, int N, int H, int W, int C, int I, const float* w1, const float* b1, const float* w2,
                           const float* b2, float* att, void* stream) {
    return splat_attn_launch(part, N, H, W, C, I, w1, b1, w2, b2, att, nullptr, nullptr, stream);
}

// the training forward: the same pass, also keeping g [N][C] (the pooled mean) and h [N][I] (fc1's post-ReLU output) for the backward
int afi_resnest_splat_attn_keep(const float* part, int N, int H, int W, int C, int I, const float* w1, const float* b1, const float* w2,
                                const float* b2, float* att, float* g, float* h, void* stream) {
    if (!g || !h) return AFI_ERR_BAD_ARG;
    if (((uintptr_t)g & 15)) return AFI_ERR_UNSUPPORTED;
    return splat_attn_launch(part, N, H, W, C, I, w1, b1, w2, b2, att, g, h, stream);
}

// out dense [N][Ho][Wo][C] = a0 * s0 + a1 * s1 per channel (avd 0: Ho = H), or its AvgPool2d(3, 2, padding 1) (avd 1: Ho = ceil(H / 2),
// divisor 9 with the zero padding counted)
__global__ __launch_bounds__(256) void afi_resnest_splat_combine_kernel(const AfiView s0, const AfiView s1, int N, int H, int W, int C,
                                                                       const float* __restrict__ att, int avd, int Ho, int Wo,
                                                                       float* __restrict__ out) {
    const int C4 = C >> 2;
    const long long total = (long long)N * Ho * Wo * C4;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % C4) * 4; long long r = i / C4;
        const int ox = (int)(r % Wo); r /= Wo; const int oy = (int)(r % Ho); const int n = (int)(r / Ho);
        const f32x4 a0 = *(const f32x4*)(att + (long long)n * 2 * C + c), a1 = *(const f32x4*)(att + (long long)n * 2 * C + C + c);
        f32x4 o;
        if (!avd) {
            o = a0 * ld4(s0, n, oy, ox, c) + a1 * ld4(s1, n, oy, ox, c);
        } else {
            f32x4 s = {0.f, 0.f, 0.f, 0.f};
            for (int ky = 0; ky < 3; ++ky) {
                const int y = 2 * oy - 1 + ky;
                if ((unsigned)y >= (unsigned)H) continue;
                for (int kx = 0; kx < 3; ++kx) {
                    const int x = 2 * ox - 1 + kx;
                    if ((unsigned)x >= (unsigned)W) continue;
                    s += a0 * ld4(s0, n, y, x, c) + a1 * ld4(s1, n, y, x, c);
                }
            }
            o = s / 9.f;
        }
        *(f32x4*)(out + i * 4) = o;
    }
}

int afi_resnest_splat_combine(afi_view_t s0, afi_view_t s1, int N, int H, int W, int C, const float* att, int avd, float* out, void* stream) {
    if (!s0.p || !s1.p || !att || !out || N <= 0 || H <= 0 || W <= 0 || C <= 0 || (avd != 0 && avd != 1)) return AFI_ERR_BAD_ARG;
    if ((C & 3) || !view_ok(s0) || !view_ok(s1) || ((uintptr_t)att & 15) || ((uintptr_t)out & 15)) return AFI_ERR_UNSUPPORTED;
    const int Ho = avd ? (H - 1) / 2 + 1 : H, Wo = avd ? (W - 1) / 2 + 1 : W;
    const AfiView v0 = {s0.p, s0.sN, s0.sH, s0.sW}, v1 = {s1.p, s1.sN, s1.sH, s1.sW};
    hipLaunchKernelGGL(afi_resnest_splat_combine_kernel, dim3(grid_of((long long)N * Ho * Wo * (C >> 2), 8192)), dim3(256), 0,
                       (hipStream_t)stream, v0, v1, N, H, W, C, att, avd, Ho, Wo, out);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}
