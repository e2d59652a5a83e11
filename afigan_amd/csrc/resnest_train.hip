// The backward of the ResNeSt bottom-up's own pieces (afigan_amd/resnest_backbone.py): split attention and the two average pools.
// The convs of a block go back through afi_conv1x1_* / afi_conv3x3_* / afi_conv3x3_wino_* and afi_frozen_wgrad_unfold, as the ResNet's do.
// Notation (radix 2): s0, s1 [N][H][W][C] the post-ReLU splits, g = mean_HW(s0 + s1), h = relu(W1' g + b1') (bn1 folded), z = W2 h + b2,
// (a0, a1) the pair softmax of z, u = a0 s0 + a1 s1, out = avd ? avg_pool(3, 2, 1)(u) : u.  du, the cotangent of u, is dout itself without AVD
// and with AVD the transposed pool of dout GATHERED: a u pixel reads the 1, 2 or 4 dout pixels whose windows hold it and divides by 9; du is
// never written to memory.
//   afi_resnest_splat_bwd_dots     per-chunk partials of sum_p du s0 and sum_p du s1 per channel, on the forward's chunks.
//   afi_resnest_splat_bwd_attn     one block per image: the partials reduced in order, dz0 = a0 a1 (da0 - da1), dz1 = -dz0,
//                                  dh = (W2^T dz) [h > 0], dg = W1'^T dh / (HW).
//   afi_resnest_splat_bwd_params   dW2 += sum_n dz_n (x) h_n, db2 += sum_n dz_n, dW1 += s1 * sum_n dh_n (x) g_n, db1 += s1 * sum_n dh_n.
//   afi_resnest_splat_bwd_combine  ds_r = (a_r du + dg) [s_r > 0], r = 0, 1, through views.
//   afi_resnest_pool_bwd           dx = beta dx + pool^T(dy) [* (z > 0)] for the two average pools, gather form.
// No atomics: every sum has one fixed order, so every kernel here is bit-identical from run to run.
#include "afi_resnest.h"

#define RS_BWD_THREADS 1024     // the per-image attention backward: 16 waves, as the forward's attention pass

typedef double f64x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f64x4 wide(f32x4 v) { return __builtin_convertvector(v, f64x4); }
__device__ __forceinline__ f32x4 narrow(f64x4 v) { return __builtin_convertvector(v, f32x4); }

static inline AfiView dev_view(const afi_view_t& v) { return AfiView{v.p, v.sN, v.sH, v.sW}; }
static inline int pooled(int n) { return (n - 1) / 2 + 1; }          // ceil(n / 2): the output size of both stride-2 pools

// du at u pixel (y, x): dout itself, or the gathered transpose of avg_pool(3, 2, 1) -- output oy covers rows 2 oy - 1 .. 2 oy + 1, so an even
// row lies in window y / 2 alone and an odd row in (y - 1) / 2 and, if it exists, (y + 1) / 2; columns alike.  Sources in ascending order.
__device__ __forceinline__ f32x4 du_at(const AfiView& d, int avd, int n, int y, int x, int c, int Ho, int Wo) {
    if (!avd) return ld4(d, n, y, x, c);
    const int oy = y >> 1, ox = x >> 1;
    const bool two_y = (y & 1) && oy + 1 < Ho, two_x = (x & 1) && ox + 1 < Wo;
    f32x4 s = ld4(d, n, oy, ox, c);
    if (two_x) s += ld4(d, n, oy, ox + 1, c);
    if (two_y) {
        s += ld4(d, n, oy + 1, ox, c);
        if (two_x) s += ld4(d, n, oy + 1, ox + 1, c);
    }
    return s / 9.f;
}

// ------------------------------------------------------------------------------------------------ dots
long long afi_resnest_splat_bwd_ws_floats(int N, int H, int W, int C) {
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || (C & 3) || C > RS_MAX_C) return 0;
    return (long long)N * gap_chunks(H, W, C) * 2 * C;
}

// part[n][k][r][c] = sum over the pixels p of chunk k (ascending by slot, then the slots in order) of du[n][p][c] * s_r[n][p][c]; grid (chunks, N).
// The products are exact in fp64 and so, to fp64 rounding, are their sums: da0 - da1 cancels in the attention pass, and what it is left with
// is then one fp32 rounding of each chunk sum, not the accumulated error of a few thousand fp32 additions.
__global__ __launch_bounds__(256) void afi_resnest_splat_bwd_dots_kernel(const AfiView dout, const AfiView s0, const AfiView s1, int H, int W,
                                                                        int C, int avd, int Ho, int Wo, int chunk_pix,
                                                                        float* __restrict__ part) {
    __shared__ f64x4 red[2][256];
    const int C4 = C >> 2, slots = 256 / C4;
    const int tid = threadIdx.x, slot = tid / C4, c = (tid % C4) * 4;
    const int k = blockIdx.x, n = blockIdx.y;
    const long long HW = (long long)H * W;
    const long long p0 = (long long)k * chunk_pix, p1 = min(p0 + chunk_pix, HW);
    f64x4 acc0 = {0., 0., 0., 0.}, acc1 = {0., 0., 0., 0.};
    if (slot < slots) {
        for (long long p = p0 + slot; p < p1; p += slots) {
            const int y = (int)(p / W), x = (int)(p % W);
            const f64x4 du = wide(du_at(dout, avd, n, y, x, c, Ho, Wo));
            acc0 += du * wide(ld4(s0, n, y, x, c));
            acc1 += du * wide(ld4(s1, n, y, x, c));
        }
    }
    red[0][tid] = acc0;
    red[1][tid] = acc1;
    __syncthreads();
    if (tid < C4) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            f64x4 s = red[r][tid];
            for (int j = 1; j < slots; ++j) s += red[r][j * C4 + tid];
            *(f32x4*)(part + (((long long)n * gridDim.x + k) * 2 + r) * C + c) = narrow(s);
        }
    }
}

int afi_resnest_splat_bwd_dots(afi_view_t dout, afi_view_t s0, afi_view_t s1, int N, int H, int W, int C, int avd, float* part,
                               long long part_floats, void* stream) {
    if (!dout.p || !s0.p || !s1.p || !part || N <= 0 || H <= 0 || W <= 0 || C <= 0 || (avd != 0 && avd != 1)) return AFI_ERR_BAD_ARG;
    if ((C & 3) || C > RS_MAX_C || !view_ok(dout) || !view_ok(s0) || !view_ok(s1) || ((uintptr_t)part & 15) || N > 65535)
        return AFI_ERR_UNSUPPORTED;
    if (part_floats < afi_resnest_splat_bwd_ws_floats(N, H, W, C)) return AFI_ERR_WORKSPACE;
    hipLaunchKernelGGL(afi_resnest_splat_bwd_dots_kernel, dim3(gap_chunks(H, W, C), N), dim3(256), 0, (hipStream_t)stream, dev_view(dout),
                       dev_view(s0), dev_view(s1), H, W, C, avd, avd ? pooled(H) : H, avd ? pooled(W) : W, gap_chunk_pix(C), part);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}

// ------------------------------------------------------------------------------------------------ attention backward, one block per image
// out[k] = sum_r v[r] * M[r][k] (v NULL: 1) for k < K, as float4 lanes by RS_BWD_THREADS / (K / 4) slots: slot j sums the rows j, j + slots, ...
// in ascending order, then the slots are added in order, all in fp64 (the work is tiny), rounded to fp32 once.  M in global memory, v and out
// in LDS; K / 4 <= RS_BWD_THREADS.
__device__ __forceinline__ void colsum_rows(const float* __restrict__ M, int R, int K, const float* v, f64x4* red, float* out) {
    const int tid = threadIdx.x, K4 = K >> 2, slots = RS_BWD_THREADS / K4, slot = tid / K4, k = (tid % K4) * 4;
    f64x4 acc = {0., 0., 0., 0.};
    if (slot < slots)
        for (int r = slot; r < R; r += slots) {
            const f64x4 m = wide(*(const f32x4*)(M + (long long)r * K + k));
            acc += v ? (double)v[r] * m : m;
        }
    red[tid] = acc;
    __syncthreads();
    if (tid < K4) {
        f64x4 s = red[tid];
        for (int j = 1; j < slots; ++j) s += red[j * K4 + tid];
        *(f32x4*)(out + k) = narrow(s);
    }
    __syncthreads();
}

// All LDS is dynamic, every carve a multiple of 16 bytes (C % 4 == 0, I % 4 == 0): red[RS_BWD_THREADS] double4, da[2C], dz[2C], dh[I], dg[C]:
// 32 KiB + (5 C + I) floats, at most 60 KiB (C <= 1024, I <= 2048).
__global__ __launch_bounds__(RS_BWD_THREADS) void afi_resnest_splat_bwd_attn_kernel(const float* __restrict__ part, int nchunk, int C, int I,
                                                                                   float hw, const float* __restrict__ att,
                                                                                   const float* __restrict__ h, const float* __restrict__ w1,
                                                                                   const float* __restrict__ w2, float* __restrict__ dz_out,
                                                                                   float* __restrict__ dh_out, float* __restrict__ dg_out) {
    extern __shared__ __attribute__((aligned(32))) char smem[];             // (a double4 slot is 32 bytes; no static LDS precedes it)
    f64x4* red = (f64x4*)smem;
    float* da = (float*)(red + RS_BWD_THREADS);
    float* dz = da + 2 * C;
    float* dh = dz + 2 * C;
    float* dg = dh + I;
    const int n = blockIdx.x, tid = threadIdx.x;
    colsum_rows(part + (long long)n * nchunk * 2 * C, nchunk, 2 * C, nullptr, red, da);
    for (int i = tid; i < C; i += RS_BWD_THREADS) {              // the pair softmax's backward: dz0 = a0 a1 (da0 - da1), dz1 = -dz0
        const float a0 = att[(long long)n * 2 * C + i], a1 = att[(long long)n * 2 * C + C + i];
        const float d = a0 * a1 * (da[i] - da[C + i]);
        dz[i] = d;
        dz[C + i] = -d;
        dz_out[(long long)n * 2 * C + i] = d;
        dz_out[(long long)n * 2 * C + C + i] = -d;
    }
    __syncthreads();
    colsum_rows(w2, 2 * C, I, dz, red, dh);                      // W2^T dz
    for (int j = tid; j < I; j += RS_BWD_THREADS) {
        const float v = h[(long long)n * I + j] > 0.f ? dh[j] : 0.f;
        dh[j] = v;
        dh_out[(long long)n * I + j] = v;
    }
    __syncthreads();
    colsum_rows(w1, I, C, dh, red, dg);                          // W1'^T dh
    for (int i = tid; i < C; i += RS_BWD_THREADS) dg_out[(long long)n * C + i] = dg[i] / hw;
}

int afi_resnest_splat_bwd_attn(const float* part, int N, int H, int W, int C, int I, const float* att, const float* h, const float* w1,
                               const float* w2, float* dz, float* dh, float* dg, void* stream) {
    if (!part || !att || !h || !w1 || !w2 || !dz || !dh || !dg || N <= 0 || H <= 0 || W <= 0 || C <= 0 || I <= 0) return AFI_ERR_BAD_ARG;
    if ((C & 3) || (I & 3) || C > RS_MAX_C || I > 2 * RS_MAX_C || ((uintptr_t)part & 15) || ((uintptr_t)w1 & 15) || ((uintptr_t)w2 & 15))
        return AFI_ERR_UNSUPPORTED;
    const size_t lds = RS_BWD_THREADS * sizeof(f64x4) + (size_t)(5 * C + I) * sizeof(float);
    hipLaunchKernelGGL(afi_resnest_splat_bwd_attn_kernel, dim3(N), dim3(RS_BWD_THREADS), lds, (hipStream_t)stream, part, gap_chunks(H, W, C), C,
                       I, (float)((double)H * W), att, h, w1, w2, dz, dh, dg);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}

// ------------------------------------------------------------------------------------------------ parameter gradients of fc1 / fc2
// One thread = one float4 of dW2 [2C][I], dW1 [I][C], db2 [2C] or db1 [I] (in that order); the images are summed in ascending order.
__global__ __launch_bounds__(256) void afi_resnest_splat_bwd_params_kernel(const float* __restrict__ dz, const float* __restrict__ dh,
                                                                          const float* __restrict__ g, const float* __restrict__ h,
                                                                          const float* __restrict__ s1, int N, int C, int I,
                                                                          float* __restrict__ dw1, float* __restrict__ db1,
                                                                          float* __restrict__ dw2, float* __restrict__ db2) {
    const int I4 = I >> 2, C4 = C >> 2;
    const long long n2 = (long long)2 * C * I4, n1 = (long long)I * C4, total = n2 + n1 + 2 * C4 + I4;
    long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (i < n2) {
        const int o = (int)(i / I4), j = (int)(i % I4) * 4;
        for (int n = 0; n < N; ++n) acc += dz[(long long)n * 2 * C + o] * *(const f32x4*)(h + (long long)n * I + j);
        *(f32x4*)(dw2 + (long long)o * I + j) += acc;
        return;
    }
    i -= n2;
    if (i < n1) {
        const int j = (int)(i / C4), c = (int)(i % C4) * 4;
        for (int n = 0; n < N; ++n) acc += dh[(long long)n * I + j] * *(const f32x4*)(g + (long long)n * C + c);
        *(f32x4*)(dw1 + (long long)j * C + c) += s1[j] * acc;
        return;
    }
    i -= n1;
    if (i < 2 * C4) {
        for (int n = 0; n < N; ++n) acc += *(const f32x4*)(dz + (long long)n * 2 * C + i * 4);
        *(f32x4*)(db2 + i * 4) += acc;
        return;
    }
    i -= 2 * C4;
    for (int n = 0; n < N; ++n) acc += *(const f32x4*)(dh + (long long)n * I + i * 4);
    *(f32x4*)(db1 + i * 4) += *(const f32x4*)(s1 + i * 4) * acc;
}

int afi_resnest_splat_bwd_params(const float* dz, const float* dh, const float* g, const float* h, const float* s1, int N, int C, int I,
                                 float* dw1, float* db1, float* dw2, float* db2, void* stream) {
    if (!dz || !dh || !g || !h || !s1 || !dw1 || !db1 || !dw2 || !db2 || N <= 0 || C <= 0 || I <= 0) return AFI_ERR_BAD_ARG;
    const uintptr_t al = (uintptr_t)dz | (uintptr_t)dh | (uintptr_t)g | (uintptr_t)h | (uintptr_t)s1 | (uintptr_t)dw1 | (uintptr_t)db1 |
                         (uintptr_t)dw2 | (uintptr_t)db2;
    if ((C & 3) || (I & 3) || C > RS_MAX_C || I > 2 * RS_MAX_C || (al & 15) || N > 65535) return AFI_ERR_UNSUPPORTED;
    const long long total = (long long)2 * C * (I >> 2) + (long long)I * (C >> 2) + 2 * (C >> 2) + (I >> 2);
    hipLaunchKernelGGL(afi_resnest_splat_bwd_params_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dz, dh, g,
                       h, s1, N, C, I, dw1, db1, dw2, db2);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}

// ------------------------------------------------------------------------------------------------ combine backward
__device__ __forceinline__ f32x4 relu_mask(f32x4 v, f32x4 z) {
    return f32x4{z.x > 0.f ? v.x : 0.f, z.y > 0.f ? v.y : 0.f, z.z > 0.f ? v.z : 0.f, z.w > 0.f ? v.w : 0.f};
}

__device__ __forceinline__ void st4(const AfiView& v, int n, int y, int x, int c, f32x4 val) {
    *(f32x4*)(v.p + n * v.sN + y * v.sH + x * v.sW + c) = val;
}

// one thread = one u pixel x 4 channels: ds_r = (a_r du + dg) [s_r > 0]
__global__ __launch_bounds__(256) void afi_resnest_splat_bwd_combine_kernel(const AfiView dout, const AfiView s0, const AfiView s1, int N, int H,
                                                                           int W, int C, const float* __restrict__ att,
                                                                           const float* __restrict__ dg, int avd, int Ho, int Wo,
                                                                           const AfiView ds0, const AfiView ds1) {
    const int C4 = C >> 2;
    const long long total = (long long)N * H * W * C4;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C4) * 4; long long r = i / C4;
    const int x = (int)(r % W); r /= W; const int y = (int)(r % H); const int n = (int)(r / H);
    const f32x4 a0 = *(const f32x4*)(att + (long long)n * 2 * C + c), a1 = *(const f32x4*)(att + (long long)n * 2 * C + C + c);
    const f32x4 g = *(const f32x4*)(dg + (long long)n * C + c);
    const f32x4 du = du_at(dout, avd, n, y, x, c, Ho, Wo);
    st4(ds0, n, y, x, c, relu_mask(a0 * du + g, ld4(s0, n, y, x, c)));
    st4(ds1, n, y, x, c, relu_mask(a1 * du + g, ld4(s1, n, y, x, c)));
}

int afi_resnest_splat_bwd_combine(afi_view_t dout, afi_view_t s0, afi_view_t s1, int N, int H, int W, int C, const float* att, const float* dg,
                                  int avd, afi_view_t ds0, afi_view_t ds1, void* stream) {
    if (!dout.p || !s0.p || !s1.p || !att || !dg || !ds0.p || !ds1.p || N <= 0 || H <= 0 || W <= 0 || C <= 0 || (avd != 0 && avd != 1))
        return AFI_ERR_BAD_ARG;
    const long long blocks = ((long long)N * H * W * (C >> 2) + 255) / 256;
    if ((C & 3) || C > RS_MAX_C || !view_ok(dout) || !view_ok(s0) || !view_ok(s1) || !view_ok(ds0) || !view_ok(ds1) || ((uintptr_t)att & 15) ||
        ((uintptr_t)dg & 15) || N > 65535 || blocks > 0x7fffffffLL)
        return AFI_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(afi_resnest_splat_bwd_combine_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, dev_view(dout),
                       dev_view(s0), dev_view(s1), N, H, W, C, att, dg, avd, avd ? pooled(H) : H, avd ? pooled(W) : W, dev_view(ds0),
                       dev_view(ds1));
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}

// ------------------------------------------------------------------------------------------------ transposed average pools
// one thread = one x pixel x 4 channels.  AVG2S2_CEIL: the pixel lies in window (y / 2, x / 2) alone, whose divisor is the pixels it covered;
// AVG3S2P1: du_at's gather.  dx is read only with beta != 0.
__global__ __launch_bounds__(256) void afi_resnest_pool_bwd_kernel(const AfiView dy, int N, int H, int W, int C, int mode, int Ho, int Wo,
                                                                  const AfiView dx, float beta, const AfiView z) {
    const int C4 = C >> 2;
    const long long total = (long long)N * H * W * C4;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C4) * 4; long long r = i / C4;
    const int x = (int)(r % W); r /= W; const int y = (int)(r % H); const int n = (int)(r / H);
    f32x4 v;
    if (mode == AFI_POOL_AVG2S2_CEIL) {
        const int oy = y >> 1, ox = x >> 1;
        v = ld4(dy, n, oy, ox, c) / (float)((min(2 * oy + 2, H) - 2 * oy) * (min(2 * ox + 2, W) - 2 * ox));
    } else {
        v = du_at(dy, 1, n, y, x, c, Ho, Wo);
    }
    if (beta != 0.f) v += beta * ld4(dx, n, y, x, c);
    if (z.p) v = relu_mask(v, ld4(z, n, y, x, c));
    st4(dx, n, y, x, c, v);
}

int afi_resnest_pool_bwd(const float* dy, int N, int H, int W, int C, int mode, afi_view_t dx, float beta, afi_view_t z_or_null, void* stream) {
    if (!dy || !dx.p || N <= 0 || H <= 0 || W <= 0 || C <= 0) return AFI_ERR_BAD_ARG;
    if (mode == AFI_POOL_MAX3S2P1) return AFI_ERR_UNSUPPORTED;                     // the max-pool's backward does not exist
    if (mode != AFI_POOL_AVG3S2P1 && mode != AFI_POOL_AVG2S2_CEIL) return AFI_ERR_BAD_ARG;
    const long long blocks = ((long long)N * H * W * (C >> 2) + 255) / 256;
    if ((C & 3) || C > RS_MAX_C || ((uintptr_t)dy & 15) || !view_ok(dx) || (z_or_null.p && !view_ok(z_or_null)) || N > 65535 ||
        blocks > 0x7fffffffLL)
        return AFI_ERR_UNSUPPORTED;
    const int Ho = pooled(H), Wo = pooled(W);
    const AfiView dyv = {const_cast<float*>(dy), (long long)Ho * Wo * C, (long long)Wo * C, (long long)C};
    hipLaunchKernelGGL(afi_resnest_pool_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, dyv, N, H, W, C, mode, Ho, Wo,
                       dev_view(dx), beta, dev_view(z_or_null));
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}
