// The kernels of the frozen Swin Transformer bottom-up (afigan_amd/swin_backbone.py) that no other launcher covers; its linears (qkv, proj
// with the residual add, fc1, fc2 with the residual add, the patch-merging reduction) run on afi_conv1x1_fwd over pixel-major tokens.
//   afi_swin_patch_embed   PatchEmbed in one pass: zero pad to a multiple of 4, Conv2d(3, C, 4, stride 4) + bias, LayerNorm; reads the NCHW
//                          batch (Cin = 3 fits no pixel-major conv) and writes pixel-major.
//   afi_swin_layernorm     LayerNorm over the channels of each pixel-major token (norm1, norm2, the output norms), or, with merge 1,
//                          PatchMerging's 2x2 gather (odd sizes zero-padded) with its LayerNorm over all 4C channels in the same pass.
//   afi_swin_gelu          exact (erf) GELU in place: the MLP's activation between fc1 and fc2.
//   afi_swin_window_attn   (shifted) window attention: one block per (window, head, image) does the gather (roll, partition, padded tokens
//                          synthesised as the qkv bias), Q K^T on the fp32 MFMA, relative-position bias, the -100 shift mask, softmax and
//                          P V, and writes each real query's result to its un-rolled, cropped pixel.
// No atomics anywhere: every sum has one fixed order, so a forward is bit-identical from run to run and under hipGraph replay.
#include "../../include/afigan_hip.h"
#include "afi_swin.h"             // the constants, grid_of, view_ok and wave_sum, shared with swin_train.hip

// ------------------------------------------------------------------------------------------------ patch embed
// x dense NCHW [N][3][H][W]; w dense [C][3][4][4]; out dense [N][Ho][Wo][C], Ho = ceil(H/4).  One wave = one output pixel: lanes 0..47 hold
// the 48 inputs of its patch (zero outside the image: the right / bottom padding), each lane 4 channels c = lane + 64 k; the weights sit in
// LDS as [patch element][C].
__global__ __launch_bounds__(256) void afi_swin_patch_embed_kernel(const float* __restrict__ x, int N, int H, int W, const float* __restrict__ w,
                                                                   const float* __restrict__ bias, const float* __restrict__ gamma,
                                                                   const float* __restrict__ beta, float eps, int C, int Ho, int Wo,
                                                                   float* __restrict__ out) {
    __shared__ float ws[48 * SW_EMBED_MAXC];
    for (int i = threadIdx.x; i < 48 * C; i += 256) ws[(i % 48) * C + i / 48] = w[i];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const long long total = (long long)N * Ho * Wo;
    for (long long pix = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); pix < total; pix += (long long)gridDim.x * 4) {
        const int ox = (int)(pix % Wo), oy = (int)((pix / Wo) % Ho), n = (int)(pix / ((long long)Wo * Ho));
        float pv = 0.f;
        if (lane < 48) {
            const int ci = lane >> 4, iy = 4 * oy + ((lane >> 2) & 3), ix = 4 * ox + (lane & 3);
            if (iy < H && ix < W) pv = x[(((long long)n * 3 + ci) * H + iy) * W + ix];
        }
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int p = 0; p < 48; ++p) {
            const float v = __shfl(pv, p, 64);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int c = lane + 64 * k;
                if (c < C) acc[k] = fmaf(v, ws[p * C + c], acc[k]);
            }
        }
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = lane + 64 * k;
            if (c < C) { acc[k] += bias[c]; s += acc[k]; }
        }
        const float mean = wave_sum(s) / (float)C;
        float q = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = lane + 64 * k;
            if (c < C) { const float d = acc[k] - mean; q += d * d; }
        }
        const float rstd = 1.f / sqrtf(wave_sum(q) / (float)C + eps);
        float* o = out + pix * C;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = lane + 64 * k;
            if (c < C) o[c] = (acc[k] - mean) * rstd * gamma[c] + beta[c];
        }
    }
}

int afi_swin_patch_embed(const float* x, int N, int H, int W, const float* w, const float* bias, const float* gamma, const float* beta, float eps,
                         int C, float* out, void* stream) {
    if (!x || !w || !bias || !gamma || !beta || !out || N <= 0 || H <= 0 || W <= 0 || C <= 0) return AFI_ERR_BAD_ARG;
    if ((C & 3) || C > SW_EMBED_MAXC) return AFI_ERR_UNSUPPORTED;
    const int Ho = (H + 3) / 4, Wo = (W + 3) / 4;
    hipLaunchKernelGGL(afi_swin_patch_embed_kernel, dim3(grid_of((long long)N * Ho * Wo, 4, 2048)), dim3(256), 0, (hipStream_t)stream, x, N, H,
                       W, w, bias, gamma, beta, eps, C, Ho, Wo, out);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}

// ------------------------------------------------------------------------------------------------ LayerNorm / patch-merging gather
// One wave = one output token of Ct channels (Ct = C, or 4C with merge), held in registers as float4s idx = lane + 64 k: two passes over
// registers (mean, then the biased variance of the centred values), one read and one write of the token.  With merge, float4 idx of the
// output token (oy, ox) is channel c = 4 idx % C of x[2 oy + (q & 1)][2 ox + (q >> 1)], q = 4 idx / C (torch.cat([x0, x1, x2, x3]) order),
// zero past the bottom / right edge.
template <int MAXV>
__global__ __launch_bounds__(256) void afi_swin_layernorm_kernel(const AfiView x, int N, int H, int W, int C, const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, float eps, int merge, int Ho, int Wo,
                                                                 float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int Ct = merge ? 4 * C : C, C4 = Ct >> 2;
    const long long total = (long long)N * Ho * Wo;
    for (long long t = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); t < total; t += (long long)gridDim.x * 4) {
        const int ox = (int)(t % Wo), oy = (int)((t / Wo) % Ho), n = (int)(t / ((long long)Wo * Ho));
        f32x4 v[MAXV];
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < MAXV; ++k) {
            const int idx = lane + 64 * k;
            v[k] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (idx < C4) {
                int y = oy, xx = ox, c = 4 * idx;
                if (merge) {
                    const int q = c / C;
                    c -= q * C; y = 2 * oy + (q & 1); xx = 2 * ox + (q >> 1);
                }
                if (y < H && xx < W) v[k] = *(const f32x4*)(x.p + n * x.sN + y * x.sH + xx * x.sW + c);
                s += (v[k].x + v[k].y) + (v[k].z + v[k].w);
            }
        }
        const float mean = wave_sum(s) / (float)Ct;
        float q = 0.f;
#pragma unroll
        for (int k = 0; k < MAXV; ++k) {
            if (lane + 64 * k < C4) {
                const f32x4 d = v[k] - mean;
                q += (d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w);
            }
        }
        const float rstd = 1.f / sqrtf(wave_sum(q) / (float)Ct + eps);
        float* o = out + t * Ct;
#pragma unroll
        for (int k = 0; k < MAXV; ++k) {
            const int idx = lane + 64 * k;
            if (idx < C4)
                *(f32x4*)(o + 4 * idx) = (v[k] - mean) * rstd * *(const f32x4*)(gamma + 4 * idx) + *(const f32x4*)(beta + 4 * idx);
        }
    }
}

int afi_swin_layernorm(afi_view_t x, int N, int H, int W, int C, const float* gamma, const float* beta, float eps, int merge, float* out,
                       void* stream) {
    if (!x.p || !gamma || !beta || !out || N <= 0 || H <= 0 || W <= 0 || C <= 0 || (merge != 0 && merge != 1)) return AFI_ERR_BAD_ARG;
    const int Ct = merge ? 4 * C : C;
    if ((C & 3) || Ct > SW_LN_MAXV * 256 || !view_ok(x) || ((uintptr_t)out & 15) || ((uintptr_t)gamma & 15) || ((uintptr_t)beta & 15))
        return AFI_ERR_UNSUPPORTED;
    const int Ho = merge ? (H + 1) / 2 : H, Wo = merge ? (W + 1) / 2 : W;
    const AfiView v = {x.p, x.sN, x.sH, x.sW};
    const dim3 grid(grid_of((long long)N * Ho * Wo, 4, 16384));
    if (Ct <= 512)                                              // registers sized to the token: occupancy of the narrow stages
        hipLaunchKernelGGL(afi_swin_layernorm_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, v, N, H, W, C, gamma, beta, eps, merge, Ho, Wo, out);
    else if (Ct <= 1536)
        hipLaunchKernelGGL(afi_swin_layernorm_kernel<6>, grid, dim3(256), 0, (hipStream_t)stream, v, N, H, W, C, gamma, beta, eps, merge, Ho, Wo, out);
    else
        hipLaunchKernelGGL(afi_swin_layernorm_kernel<SW_LN_MAXV>, grid, dim3(256), 0, (hipStream_t)stream, v, N, H, W, C, gamma, beta, eps, merge, Ho,
                           Wo, out);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}

// ------------------------------------------------------------------------------------------------ GELU
__global__ __launch_bounds__(256) void afi_swin_gelu_kernel(float* __restrict__ x, long long n4) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        f32x4 v = *(f32x4*)(x + 4 * i);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = 0.5f * v[j] * (1.f + erff(v[j] * 0.70710678118654752f));
        *(f32x4*)(x + 4 * i) = v;
    }
}

int afi_swin_gelu(float* x, long long n, void* stream) {
    if (!x || n < 0) return AFI_ERR_BAD_ARG;
    if ((n & 3) || ((uintptr_t)x & 15)) return AFI_ERR_UNSUPPORTED;
    if (n == 0) return AFI_OK;
    hipLaunchKernelGGL(afi_swin_gelu_kernel, dim3(grid_of(n / 4, 256, 16384)), dim3(256), 0, (hipStream_t)stream, x, n / 4);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}

// ------------------------------------------------------------------------------------------------ window attention
// Block (window, head, image), one wave per 16 query rows of the window (NT = ceil(WS^2 / 16) waves: 4 for WS 7, 9 for WS 12).
// Window token t (row t / WS, column t % WS of the window at (wy0, wx0) of the rolled, padded Hp x Wp map) is pixel
// ((wy0 + t / WS + shift) % Hp, (wx0 + t % WS + shift) % Wp) of the un-rolled map: torch.roll(x, -shift) then window_partition.  A pixel
// outside H x W is a padded token: its q / k / v are the qkv bias exactly (norm1 runs before the zero padding).  Tokens t >= WS^2 (the tile
// padding) are zero and are excluded from every softmax.  The kernel states this roll / region rule inline; afi_swin.h's swin_window_token is the
// same rule for the backward kernels of swin_train.hip: a change to one is a change to both.
// With the f32 MFMA 16x16x4 (A[l & 15][l >> 4], B[l >> 4][l & 15], D col l & 15, row 4 (l >> 4) + r) the wave computes S^T = K Q^T, so lane
// l holds the scores of query i = 16 ti + (l & 15) against keys 16 tj + 4 (l >> 4) + r: a softmax row is spread over 4 lanes (shfl_xor 16,
// 32), and the probabilities, in registers, are already the A operand of O = P V (k step (tj, r) <-> keys 16 tj + 4 k + r).
template <int WS>
__global__ __launch_bounds__(((WS * WS + 15) / 16) * 64) void afi_swin_attn_kernel(const AfiView qkv, int H, int W, int C, int Hp, int Wp,
                                                                                   const float* __restrict__ qkv_bias,
                                                                                   const float* __restrict__ bias_img, int shift,
                                                                                   float* __restrict__ out) {
    constexpr int NW = WS * WS, NT = (NW + 15) / 16, NP = 16 * NT, LD = SW_LDS_LD, D = SW_HEAD_DIM;
    __shared__ f32x4 lds4[3 * NP * LD / 4];
    __shared__ int spy[NP], spx[NP], sreg[NP];
    float* sq = (float*)lds4;
    float* sk = sq + NP * LD;
    float* sv = sk + NP * LD;
    const int nWw = Wp / WS;
    const int win = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int wy0 = (win / nWw) * WS, wx0 = (win % nWw) * WS;
    const float scale = 0.17677669529663687f;                   // 32^-0.5

    for (int t = threadIdx.x; t < NP; t += NT * 64) {
        int py = -1, px = -1, reg = 0;
        if (t < NW) {
            const int ry = wy0 + t / WS, rx = wx0 + t % WS;
            py = (ry + shift) % Hp; px = (rx + shift) % Wp;
            if (py >= H || px >= W) py = px = -1;
            if (shift) reg = 3 * (ry < Hp - WS ? 0 : (ry < Hp - shift ? 1 : 2)) + (rx < Wp - WS ? 0 : (rx < Wp - shift ? 1 : 2));
        }
        spy[t] = py; spx[t] = px; sreg[t] = reg;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < NP * 24; e += NT * 64) {
        const int t = e / 24, s = (e % 24) >> 3, d4 = (e & 7) * 4;
        const int ch = s * C + h * D + d4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (t < NW) {
            const int py = spy[t], px = spx[t];
            v = py >= 0 ? *(const f32x4*)(qkv.p + b * qkv.sN + py * qkv.sH + px * qkv.sW + ch) : *(const f32x4*)(qkv_bias + ch);
        }
        if (s == 0) v *= scale;
        *(f32x4*)(sq + s * NP * LD + t * LD + d4) = v;
    }
    __syncthreads();

    const int lane = threadIdx.x & 63, ti = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
    const int qi = 16 * ti + li;                                // this lane's query in the score layout
    if (!__any(qi < NW && spy[qi] >= 0)) return;               // a strip of padded / tile-padding queries only: all of it is cropped

    float qf[D / 4];
#pragma unroll
    for (int s = 0; s < D / 4; ++s) qf[s] = sq[qi * LD + 4 * s + lk];
    f32x4_mfma st[NT];
#pragma unroll
    for (int tj = 0; tj < NT; ++tj) {
        f32x4_mfma acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < D / 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(sk[(16 * tj + li) * LD + 4 * s + lk], qf[s], acc, 0, 0, 0);
        st[tj] = acc;
    }
    // + relative-position bias (dense [heads][NP][NP] image), + the shift mask, softmax over the keys j < NW
    const float* brow = bias_img + ((long long)h * NP + qi) * NP;
    const int regi = sreg[qi];
    float m = -INFINITY;
#pragma unroll
    for (int tj = 0; tj < NT; ++tj) {
        const int j0 = 16 * tj + 4 * lk;
        const f32x4 bb = *(const f32x4*)(brow + j0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float v = st[tj][r] + bb[r];
            if (shift && sreg[j0 + r] != regi) v += -100.f;
            if (j0 + r >= NW) v = -INFINITY;
            st[tj][r] = v;
            m = fmaxf(m, v);
        }
    }
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    float sum = 0.f;
#pragma unroll
    for (int tj = 0; tj < NT; ++tj)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float e = expf(st[tj][r] - m);
            st[tj][r] = e;
            sum += e;
        }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    const float inv = 1.f / sum;
#pragma unroll
    for (int tj = 0; tj < NT; ++tj) st[tj] *= inv;

    // O = P V, two 16-column tiles of the head; D row 4 lk + r = query 16 ti + 4 lk + r, column li = head channel 16 dt + li
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt) {
        f32x4_mfma acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int tj = 0; tj < NT; ++tj)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(st[tj][r], sv[(16 * tj + 4 * lk + r) * LD + 16 * dt + li], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int t = 16 * ti + 4 * lk + r;
            if (t < NW && spy[t] >= 0)
                out[(((long long)b * H + spy[t]) * W + spx[t]) * C + h * D + 16 * dt + li] = acc[r];
        }
    }
}

int afi_swin_window_attn(afi_view_t qkv, int N, int H, int W, int C, const float* qkv_bias, const float* bias_img, int window, int shift,
                         float* out, void* stream) {
    if (!qkv.p || !qkv_bias || !bias_img || !out || N <= 0 || H <= 0 || W <= 0 || C <= 0 || shift < 0 || shift >= window) return AFI_ERR_BAD_ARG;
    if (C % SW_HEAD_DIM || !view_ok(qkv) || ((uintptr_t)qkv_bias & 15) || ((uintptr_t)bias_img & 15) || N > 65535) return AFI_ERR_UNSUPPORTED;
    if (window != 7 && window != 12) return AFI_ERR_UNSUPPORTED;
    const int Hp = (H + window - 1) / window * window, Wp = (W + window - 1) / window * window;
    const dim3 grid((unsigned)((Hp / window) * (Wp / window)), (unsigned)(C / SW_HEAD_DIM), (unsigned)N);
    const AfiView v = {qkv.p, qkv.sN, qkv.sH, qkv.sW};
    if (window == 7)
        hipLaunchKernelGGL(afi_swin_attn_kernel<7>, grid, dim3(4 * 64), 0, (hipStream_t)stream, v, H, W, C, Hp, Wp, qkv_bias, bias_img, shift, out);
    else
        hipLaunchKernelGGL(afi_swin_attn_kernel<12>, grid, dim3(9 * 64), 0, (hipStream_t)stream, v, H, W, C, Hp, Wp, qkv_bias, bias_img, shift, out);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}
