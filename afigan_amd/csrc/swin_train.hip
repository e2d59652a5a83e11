// The backward kernels of the Swin Transformer bottom-up (afigan_amd/swin_backbone.py, _SwinTrainFn).  The linears' gradients run
// on afi_conv1x1_dgrad / afi_conv1x1_wgrad / afi_colsum_accum; these cover the rest.
//   afi_swin_layernorm_bwd    dx (fresh or added into a gradient, for merge 1 scattered to the four source pixels) and per-wave partial sums of
//                             d gamma / d beta, which afi_swin_ln_params_kernel adds in ascending order in fp64 and += into the gradients.
//   afi_swin_gelu_bwd         dx = dy (Phi(x) + x phi(x)).
//   afi_swin_window_attn_bwd  one block per (group of windows, head, image): recomputes S and P as the forward does, dq / dk / dv of every
//                             padded-map position into a [N][Hp][Wp][3C] buffer, and the block's sum of dS into a workspace.
//   afi_swin_bias_table_bwd   one wave per (table row, head): the dS partials of the pairs that index the row, in fp64, += into the table's gradient.
//   afi_swin_patch_gather     the zero-padded 4x4x3 patches of an NCHW batch as pixel-major [N][Ho][Wo][48].
//   afi_swin_scale_add        out = a + s[n] b (DropPath).
// No atomics: every sum has one fixed order, so a backward is bit-identical from run to run.
#include "../../include/afigan_hip.h"
#include "afi_swin.h"

#include <map>
#include <mutex>

// ------------------------------------------------------------------------------------------------ LayerNorm backward
#define SW_LNB_TOKENS 8         // tokens per wave the grid is sized for (more when the grid cap binds)
#define SW_LNB_GRID_CAP 1024

static inline unsigned lnb_grid(long long tokens) { return grid_of(tokens, 4 * SW_LNB_TOKENS, SW_LNB_GRID_CAP); }

// One wave = one token of Ct channels as in afi_swin_layernorm_kernel: x-hat and rstd are recomputed from the forward's input with the forward's
// arithmetic.  g = dy gamma;  dx = rstd (g - mean(g) - x-hat mean(g x-hat)).  Each lane keeps sum dy x-hat and sum dy of its channels over the
// wave's tokens; the wave writes them as row (4 block + wave) of part [rows][2][Ct].
template <int MAXV>
__global__ __launch_bounds__(256) void afi_swin_layernorm_bwd_kernel(const AfiView x, int N, int H, int W, int C, const float* __restrict__ gamma,
                                                                     float eps, int merge, int Ho, int Wo, const float* __restrict__ dy,
                                                                     const AfiView dx, float beta, float* __restrict__ part) {
    const int lane = threadIdx.x & 63;
    const int Ct = merge ? 4 * C : C, C4 = Ct >> 2;
    const long long total = (long long)N * Ho * Wo;
    f32x4 ag[MAXV], ab[MAXV];
#pragma unroll
    for (int k = 0; k < MAXV; ++k) ag[k] = ab[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (long long t = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); t < total; t += (long long)gridDim.x * 4) {
        const int ox = (int)(t % Wo), oy = (int)((t / Wo) % Ho), n = (int)(t / ((long long)Wo * Ho));
        f32x4 v[MAXV], g[MAXV];
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
        const float* gy = dy + t * Ct;
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int k = 0; k < MAXV; ++k) {
            const int idx = lane + 64 * k;
            g[k] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (idx < C4) {
                const f32x4 d = *(const f32x4*)(gy + 4 * idx);
                const f32x4 xh = (v[k] - mean) * rstd;
                ab[k] += d;
                ag[k] += d * xh;
                g[k] = d * *(const f32x4*)(gamma + 4 * idx);
                v[k] = xh;
                const f32x4 gx = g[k] * xh;
                s1 += (g[k].x + g[k].y) + (g[k].z + g[k].w);
                s2 += (gx.x + gx.y) + (gx.z + gx.w);
            }
        }
        const float m1 = wave_sum(s1) / (float)Ct, m2 = wave_sum(s2) / (float)Ct;
        if (dx.p) {
#pragma unroll
            for (int k = 0; k < MAXV; ++k) {
                const int idx = lane + 64 * k;
                if (idx < C4) {
                    int y = oy, xx = ox, c = 4 * idx;
                    if (merge) {
                        const int qd = c / C;
                        c -= qd * C; y = 2 * oy + (qd & 1); xx = 2 * ox + (qd >> 1);
                    }
                    if (y < H && xx < W) {                      // a quadrant past an odd bottom / right edge has no source pixel: dropped
                        f32x4 r = (g[k] - m1 - v[k] * m2) * rstd;
                        float* o = dx.p + n * dx.sN + y * dx.sH + xx * dx.sW + c;
                        if (beta != 0.f) r += *(const f32x4*)o * beta;
                        *(f32x4*)o = r;
                    }
                }
            }
        }
    }
    if (part) {
        float* row = part + ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 2 * Ct;
#pragma unroll
        for (int k = 0; k < MAXV; ++k) {
            const int idx = lane + 64 * k;
            if (idx < C4) {
                *(f32x4*)(row + 4 * idx) = ag[k];
                *(f32x4*)(row + Ct + 4 * idx) = ab[k];
            }
        }
    }
}

// Block = 16 columns (which, c) of part's rows x 16 slices of consecutive rows.  Thread (column, slice) adds its slice's rows in ascending order
// in fp64; the 16 slice sums are then added in ascending order, rounded once and added to the parameter's gradient: one fixed order, a
// function of `rows` alone.  (One thread per column over all rows is the same sum at 1 / 20 of the speed: 4096 dependent rows on 3 blocks.)
#define SW_LNP_COLS 16
#define SW_LNP_SLICES 16
__global__ __launch_bounds__(SW_LNP_COLS * SW_LNP_SLICES) void afi_swin_ln_params_kernel(const float* __restrict__ part, int rows, int Ct,
                                                                                         float* __restrict__ dgamma, float* __restrict__ dbeta) {
    __shared__ double sums[SW_LNP_SLICES][SW_LNP_COLS];
    const int col = threadIdx.x % SW_LNP_COLS, sl = threadIdx.x / SW_LNP_COLS;
    const int i = blockIdx.x * SW_LNP_COLS + col;                // column of a [rows][2 Ct] matrix: dgamma's Ct, then dbeta's
    const int per = (rows + SW_LNP_SLICES - 1) / SW_LNP_SLICES;
    const int r0 = sl * per, r1 = r0 + per < rows ? r0 + per : rows;
    double acc = 0.0;
    if (i < 2 * Ct) {
#pragma unroll 8
        for (int r = r0; r < r1; ++r) acc += (double)part[(long long)r * 2 * Ct + i];
    }
    sums[sl][col] = acc;
    __syncthreads();
    if (sl == 0 && i < 2 * Ct) {
        double total = 0.0;
#pragma unroll
        for (int s = 0; s < SW_LNP_SLICES; ++s) total += sums[s][col];
        float* dst = i < Ct ? dgamma : dbeta;
        dst[i < Ct ? i : i - Ct] += (float)total;
    }
}

int afi_swin_layernorm_bwd_vecs(int Ct) {
    if (Ct <= 0 || (Ct & 3) || Ct > SW_LN_MAXV * 256) return -1;
    return Ct <= 512 ? 2 : (Ct <= 1536 ? 6 : SW_LN_MAXV);
}

long long afi_swin_layernorm_bwd_ws_floats(int N, int H, int W, int C, int merge) {
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || (merge != 0 && merge != 1)) return -1;
    const int Ho = merge ? (H + 1) / 2 : H, Wo = merge ? (W + 1) / 2 : W;
    return (long long)lnb_grid((long long)N * Ho * Wo) * 4 * 2 * (merge ? 4 * C : C);
}

int afi_swin_layernorm_bwd(afi_view_t x, int N, int H, int W, int C, const float* gamma, float eps, int merge, const float* dy, afi_view_t dx,
                           float beta, float* dgamma, float* dbeta, float* ws, long long ws_floats, void* stream) {
    if (!x.p || !gamma || !dy || N <= 0 || H <= 0 || W <= 0 || C <= 0 || (merge != 0 && merge != 1) || (!dgamma) != (!dbeta) ||
        (!dx.p && !dgamma))
        return AFI_ERR_BAD_ARG;
    const int Ct = merge ? 4 * C : C;
    if ((C & 3) || Ct > SW_LN_MAXV * 256 || !view_ok(x) || (dx.p && !view_ok(dx)) || ((uintptr_t)dy & 15) || ((uintptr_t)gamma & 15) ||
        ((uintptr_t)ws & 15))
        return AFI_ERR_UNSUPPORTED;
    const long long need = afi_swin_layernorm_bwd_ws_floats(N, H, W, C, merge);
    if (dgamma && (!ws || ws_floats < need)) return AFI_ERR_WORKSPACE;
    const int Ho = merge ? (H + 1) / 2 : H, Wo = merge ? (W + 1) / 2 : W;
    const AfiView v = {x.p, x.sN, x.sH, x.sW}, dv = {dx.p, dx.sN, dx.sH, dx.sW};
    const dim3 grid(lnb_grid((long long)N * Ho * Wo));
    float* part = dgamma ? ws : nullptr;
    const int vecs = afi_swin_layernorm_bwd_vecs(Ct);
    if (vecs == 2)
        hipLaunchKernelGGL(afi_swin_layernorm_bwd_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, v, N, H, W, C, gamma, eps, merge, Ho, Wo, dy,
                           dv, beta, part);
    else if (vecs == 6)
        hipLaunchKernelGGL(afi_swin_layernorm_bwd_kernel<6>, grid, dim3(256), 0, (hipStream_t)stream, v, N, H, W, C, gamma, eps, merge, Ho, Wo, dy,
                           dv, beta, part);
    else
        hipLaunchKernelGGL(afi_swin_layernorm_bwd_kernel<SW_LN_MAXV>, grid, dim3(256), 0, (hipStream_t)stream, v, N, H, W, C, gamma, eps, merge, Ho,
                           Wo, dy, dv, beta, part);
    if (hipGetLastError() != hipSuccess) return AFI_ERR_LAUNCH;
    if (dgamma) {
        hipLaunchKernelGGL(afi_swin_ln_params_kernel, dim3((2 * Ct + SW_LNP_COLS - 1) / SW_LNP_COLS), dim3(SW_LNP_COLS * SW_LNP_SLICES), 0,
                           (hipStream_t)stream, part, (int)grid.x * 4, Ct, dgamma, dbeta);
        if (hipGetLastError() != hipSuccess) return AFI_ERR_LAUNCH;
    }
    return AFI_OK;
}

// ------------------------------------------------------------------------------------------------ GELU backward
__global__ __launch_bounds__(256) void afi_swin_gelu_bwd_kernel(const float* __restrict__ x, const float* dy, float* dx, long long n4) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const f32x4 v = *(const f32x4*)(x + 4 * i);
        f32x4 g = *(const f32x4*)(dy + 4 * i);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float cdf = 0.5f * (1.f + erff(v[j] * 0.70710678118654752f));
            const float pdf = expf(-0.5f * v[j] * v[j]) * 0.39894228040143268f;
            g[j] *= cdf + v[j] * pdf;
        }
        *(f32x4*)(dx + 4 * i) = g;
    }
}

int afi_swin_gelu_bwd(const float* x, const float* dy, float* dx, long long n, void* stream) {
    if (!x || !dy || !dx || n < 0) return AFI_ERR_BAD_ARG;
    if ((n & 3) || ((uintptr_t)x & 15) || ((uintptr_t)dy & 15) || ((uintptr_t)dx & 15)) return AFI_ERR_UNSUPPORTED;
    if (n == 0) return AFI_OK;
    hipLaunchKernelGGL(afi_swin_gelu_bwd_kernel, dim3(grid_of(n / 4, 256, 16384)), dim3(256), 0, (hipStream_t)stream, x, dy, dx, n / 4);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}

// ------------------------------------------------------------------------------------------------ window attention backward
// Block (group of `wpb` consecutive windows, head, image), NT waves, the forward's LDS tiles (q scaled, k, v) plus dO.  Per window:
//   phase A  wave ti owns queries 16 ti ..: S^T = K Q^T and P exactly as afi_swin_attn_kernel (same operands, same order); rs = rowsum(dP P)
//            as dO . (P V), which needs no dP tile kept; the row's max, 1 / sum and rs go to LDS.  Then per key tile dP^T = V dO^T in the
//            score layout, dS = P (dP - rs), added to the block's running sum over its windows (its slice of ds_part) and, as the A operand of the
//            MFMA, into dQ = 32^-1/2 dS K.
//   phase B  wave tw owns keys 16 tw ..: per query tile S = Q K^T (the transposed tile: key per lane, 4 queries per register), P from the
//            stored max and 1 / sum, dP = dO V^T, dS; dV += P^T dO and dK += dS^T (32^-1/2 Q), both with the tile as the A operand.
// dq / dk / dv are written for EVERY token of the window -- a padded token's q / k / v are the qkv bias, so its gradient is the bias's -- at
// its un-rolled position of the padded map: each position belongs to one window, a plain store.  Queries that are padding have dO = 0, hence
// dS rows of zero; their keys and values still receive gradient from the real queries, so no strip is skipped.
template <int WS>
__global__ __launch_bounds__(((WS * WS + 15) / 16) * 64) void afi_swin_attn_bwd_kernel(const AfiView qkv, const AfiView dout, int H, int W, int C,
                                                                                       int Hp, int Wp, const float* qkv_bias, const float* bias_img,
                                                                                       int shift, int wpb, float* dqkv, float* ds_part) {
    // (no __restrict__: the bias rows are the same for every window of the block, and hoisting their 36 registers out of the window loop is
    // what the window-12 instantiation has no room for)
    constexpr int NW = WS * WS, NT = (NW + 15) / 16, NP = 16 * NT, LD = SW_LDS_LD, D = SW_HEAD_DIM;
    extern __shared__ __attribute__((aligned(16))) float sw_lds[];     // dynamic only: 86400 bytes for WS 12 (no static LDS in front of it)
    float* sq = sw_lds;
    float* sk = sq + NP * LD;
    float* sv = sk + NP * LD;
    float* sdo = sv + NP * LD;
    float* smax = sdo + NP * LD;
    float* sinv = smax + NP;
    float* srs = sinv + NP;
    int* spos = (int*)(srs + NP);                               // py * Wp + px of the token in the padded map; -1: tile padding
    int* sreal = spos + NP;                                     // 1: a pixel inside H x W
    int* sreg = sreal + NP;
    const int nWw = Wp / WS, nW = (Hp / WS) * nWw;
    const int grp = blockIdx.x, h = blockIdx.y, b = blockIdx.z, heads = gridDim.y;
    const float scale = 0.17677669529663687f;                   // 32^-0.5
    const int lane = threadIdx.x & 63, ti = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
    const int qi = 16 * ti + li;
    const long long C3 = 3LL * C;
    float* dbase = dqkv + (long long)b * Hp * Wp * C3 + h * D;

    // the block's sum of dS over its windows: [image][group][head][NP][NP], row = query, 4 keys per lane; the first window stores, the
    // later ones add to what this same lane stored (registers are short in the window-12 instantiation)
    float* dsimg = ds_part + (((long long)b * gridDim.x + grp) * heads + h) * NP * NP;

    const int win_end = (grp + 1) * wpb < nW ? (grp + 1) * wpb : nW;
    for (int win = grp * wpb; win < win_end; ++win) {
        const int wy0 = (win / nWw) * WS, wx0 = (win % nWw) * WS;
        for (int t = threadIdx.x; t < NP; t += NT * 64) {
            int pos = -1, real = 0, reg = 0;
            if (t < NW) {
                int py, px;
                swin_window_token(t, WS, wy0, wx0, Hp, Wp, shift, py, px, reg);
                pos = py * Wp + px;
                real = py < H && px < W;
            }
            spos[t] = pos; sreal[t] = real; sreg[t] = reg;
        }
        __syncthreads();
        for (int e = threadIdx.x; e < NP * 32; e += NT * 64) {
            const int t = e >> 5, s = (e & 31) >> 3, d4 = (e & 7) * 4;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (t < NW) {
                const int pos = spos[t], py = pos / Wp, px = pos - py * Wp;
                if (s < 3) {
                    const int ch = s * C + h * D + d4;
                    v = sreal[t] ? *(const f32x4*)(qkv.p + b * qkv.sN + py * qkv.sH + px * qkv.sW + ch) : *(const f32x4*)(qkv_bias + ch);
                } else if (sreal[t]) {
                    v = *(const f32x4*)(dout.p + b * dout.sN + py * dout.sH + px * dout.sW + h * D + d4);
                }
            }
            if (s == 0) v *= scale;
            *(f32x4*)(sq + s * NP * LD + t * LD + d4) = v;
        }
        __syncthreads();

        // ---- phase A: this wave's 16 queries
        {
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
                __builtin_amdgcn_sched_barrier(0);
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

            // rs[i] = rowsum(dP P) = dO[i] . O[i]: O = P V as the forward forms it (row 4 lk + r = query 16 ti + 4 lk + r, column li = channel),
            // dotted with dO over the 16 lanes of a row; through LDS into the score layout (query per lane)
            float rsr[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int dt = 0; dt < D / 16; ++dt) {
                f32x4_mfma acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int tj = 0; tj < NT; ++tj) {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(st[tj][r], sv[(16 * tj + 4 * lk + r) * LD + 16 * dt + li], acc, 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) rsr[r] = fmaf(acc[r], sdo[(16 * ti + 4 * lk + r) * LD + 16 * dt + li], rsr[r]);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) rsr[r] += __shfl_xor(rsr[r], o, 64);
                if (li == 0) srs[16 * ti + 4 * lk + r] = rsr[r];
            }
            if (lk == 0) { smax[qi] = m; sinv[qi] = inv; }
            __syncthreads();                                    // the rows' max, 1 / sum and rs: read below and by every wave in phase B
            const float rs = srs[qi];
            float dof[D / 4];
#pragma unroll
            for (int s = 0; s < D / 4; ++s) dof[s] = sdo[qi * LD + 4 * s + lk];
            // per key tile: dP^T = V dO^T, dS = P (dP - rs), into the block's sum and, as the A operand, into dQ = scale dS K
            // (D row 4 lk + r = query 16 ti + 4 lk + r, column li = head channel 16 dt + li)
            f32x4_mfma dq[D / 16];
#pragma unroll
            for (int dt = 0; dt < D / 16; ++dt) dq[dt] = f32x4_mfma{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int tj = 0; tj < NT; ++tj) {
                f32x4_mfma dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s = 0; s < D / 4; ++s) dp = __builtin_amdgcn_mfma_f32_16x16x4f32(sv[(16 * tj + li) * LD + 4 * s + lk], dof[s], dp, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; ++r) dp[r] = st[tj][r] * (dp[r] - rs);               // dS
                {
                    f32x4 cur = {dp[0], dp[1], dp[2], dp[3]};
                    float* o = dsimg + (qi * NP + 16 * tj + 4 * lk);
                    if (win > grp * wpb) cur += *(const f32x4*)o;
                    *(f32x4*)o = cur;
                }
#pragma unroll
                for (int dt = 0; dt < D / 16; ++dt)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        dq[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(dp[r], sk[(16 * tj + 4 * lk + r) * LD + 16 * dt + li], dq[dt], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);              // one key tile's operands in flight at a time: the window-12 instantiation has 168 VGPRs
            }
#pragma unroll
            for (int dt = 0; dt < D / 16; ++dt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int t = 16 * ti + 4 * lk + r;
                    if (t < NW) dbase[spos[t] * C3 + 16 * dt + li] = dq[dt][r] * scale;
                }
        }

        // ---- phase B: this wave's 16 keys (lane: key 16 ti + li; register r of tile tq: query 16 tq + 4 lk + r)
        {
            const int kj = 16 * ti + li;
            const int regk = sreg[kj];
            float kf[D / 4], vf[D / 4];
#pragma unroll
            for (int s = 0; s < D / 4; ++s) { kf[s] = sk[kj * LD + 4 * s + lk]; vf[s] = sv[kj * LD + 4 * s + lk]; }
            f32x4_mfma dk[D / 16], dvv[D / 16];
#pragma unroll
            for (int dt = 0; dt < D / 16; ++dt) dk[dt] = dvv[dt] = f32x4_mfma{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
            for (int tq = 0; tq < NT; ++tq) {
                f32x4_mfma sc = {0.f, 0.f, 0.f, 0.f}, dpt = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s = 0; s < D / 4; ++s) {
                    sc = __builtin_amdgcn_mfma_f32_16x16x4f32(sq[(16 * tq + li) * LD + 4 * s + lk], kf[s], sc, 0, 0, 0);
                    dpt = __builtin_amdgcn_mfma_f32_16x16x4f32(sdo[(16 * tq + li) * LD + 4 * s + lk], vf[s], dpt, 0, 0, 0);
                }
                f32x4_mfma p, dsv;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = 16 * tq + 4 * lk + r;
                    float v = sc[r] + bias_img[((long long)h * NP + i) * NP + kj];
                    if (shift && sreg[i] != regk) v += -100.f;
                    const float pr = kj < NW ? expf(v - smax[i]) * sinv[i] : 0.f;
                    p[r] = pr;
                    dsv[r] = pr * (dpt[r] - srs[i]);
                }
#pragma unroll
                for (int dt = 0; dt < D / 16; ++dt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int i = 16 * tq + 4 * lk + r;
                        dvv[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(p[r], sdo[i * LD + 16 * dt + li], dvv[dt], 0, 0, 0);
                        dk[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(dsv[r], sq[i * LD + 16 * dt + li], dk[dt], 0, 0, 0);
                    }
            }
#pragma unroll
            for (int dt = 0; dt < D / 16; ++dt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int t = 16 * ti + 4 * lk + r;
                    if (t < NW) {
                        float* o = dbase + spos[t] * C3 + 16 * dt + li;
                        o[C] = dk[dt][r];
                        o[2 * C] = dvv[dt][r];
                    }
                }
        }
        __syncthreads();                                        // the tiles are rewritten for the next window
    }
}

// windows per block: one while the grid stays small, more (at most 8) to shrink the dS workspace of the large maps; a function of the shape only
static inline int attn_bwd_wpb(int N, int nW, int heads) {
    const long long blocks = (long long)N * nW * heads;
    const long long w = blocks / 1024;
    return w < 1 ? 1 : (w > 8 ? 8 : (int)w);
}

static bool attn_bwd_lds_ok(const void* fn, int bytes) {
    static std::mutex mu;
    static std::map<std::pair<int, const void*>, bool> done;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return false;
    std::lock_guard<std::mutex> lock(mu);
    if (done.count({dev, fn})) return true;
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return false;
    done[{dev, fn}] = true;
    return true;
}

long long afi_swin_window_attn_bwd_ws_floats(int N, int H, int W, int C, int window) {
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || C % SW_HEAD_DIM || (window != 7 && window != 12)) return -1;
    const int nW = ((H + window - 1) / window) * ((W + window - 1) / window), heads = C / SW_HEAD_DIM;
    const int wpb = attn_bwd_wpb(N, nW, heads), NP = (window * window + 15) / 16 * 16;
    return (long long)N * ((nW + wpb - 1) / wpb) * heads * NP * NP;
}

long long afi_swin_window_attn_bwd_groups(int N, int H, int W, int C, int window) {
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || C % SW_HEAD_DIM || (window != 7 && window != 12)) return -1;
    const int nW = ((H + window - 1) / window) * ((W + window - 1) / window);
    const int wpb = attn_bwd_wpb(N, nW, C / SW_HEAD_DIM);
    return (nW + wpb - 1) / wpb;
}

int afi_swin_window_attn_bwd(afi_view_t qkv, afi_view_t dout, int N, int H, int W, int C, const float* qkv_bias, const float* bias_img, int window,
                             int shift, float* dqkv, float* ds_part, long long ds_floats, void* stream) {
    if (!qkv.p || !dout.p || !qkv_bias || !bias_img || !dqkv || !ds_part || N <= 0 || H <= 0 || W <= 0 || C <= 0 || shift < 0 || shift >= window)
        return AFI_ERR_BAD_ARG;
    if (C % SW_HEAD_DIM || !view_ok(qkv) || !view_ok(dout) || ((uintptr_t)qkv_bias & 15) || ((uintptr_t)bias_img & 15) || ((uintptr_t)ds_part & 15) ||
        N > 65535)
        return AFI_ERR_UNSUPPORTED;
    if (window != 7 && window != 12) return AFI_ERR_UNSUPPORTED;
    const int Hp = (H + window - 1) / window * window, Wp = (W + window - 1) / window * window;
    if ((long long)Hp * Wp * 3 * C >= (1LL << 31)) return AFI_ERR_UNSUPPORTED;      // a position's offset in one image of dqkv is an int
    if (ds_floats < afi_swin_window_attn_bwd_ws_floats(N, H, W, C, window)) return AFI_ERR_WORKSPACE;
    const int nW = (Hp / window) * (Wp / window), heads = C / SW_HEAD_DIM, wpb = attn_bwd_wpb(N, nW, heads);
    const dim3 grid((unsigned)((nW + wpb - 1) / wpb), (unsigned)heads, (unsigned)N);
    const AfiView v = {qkv.p, qkv.sN, qkv.sH, qkv.sW}, dv = {dout.p, dout.sN, dout.sH, dout.sW};
    const int NP = (window * window + 15) / 16 * 16;
    const int lds = (4 * NP * SW_LDS_LD + 6 * NP) * 4;
    if (window == 7) {
        if (!attn_bwd_lds_ok((const void*)afi_swin_attn_bwd_kernel<7>, lds)) return AFI_ERR_LAUNCH;
        hipLaunchKernelGGL(afi_swin_attn_bwd_kernel<7>, grid, dim3(4 * 64), lds, (hipStream_t)stream, v, dv, H, W, C, Hp, Wp, qkv_bias, bias_img, shift,
                           wpb, dqkv, ds_part);
    } else {
        if (!attn_bwd_lds_ok((const void*)afi_swin_attn_bwd_kernel<12>, lds)) return AFI_ERR_LAUNCH;
        hipLaunchKernelGGL(afi_swin_attn_bwd_kernel<12>, grid, dim3(9 * 64), lds, (hipStream_t)stream, v, dv, H, W, C, Hp, Wp, qkv_bias, bias_img,
                           shift, wpb, dqkv, ds_part);
    }
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}

// ------------------------------------------------------------------------------------------------ relative-position bias table gradient
// Two passes over a workspace `img` of heads NP NP doubles.  Pass 1, thread per (h, i, j): the partials of ds_part [nparts][heads][NP][NP]
// (image-major, then group of windows) in ascending order, in fp64 -- neighbouring lanes read neighbouring floats.  Pass 2, one wave per (table
// row r, head h): row_off [R + 1] / pairs is the CSR of relative_position_index as loaded -- pairs[p] = i NP + j of the (i, j) with
// index[i][j] = r, ascending; lane l takes the pairs l, l + 64, ... of the row from the 8 heads NP NP bytes of `img`, the lanes are joined by a
// fixed xor tree, and dtable[r][h] += the sum rounded once.
__global__ __launch_bounds__(256) void afi_swin_bias_sum_parts_kernel(const float* __restrict__ ds_part, int nparts, long long per_part,
                                                                      double* __restrict__ img) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= per_part) return;
    double acc = 0.0;
#pragma unroll 4
    for (int part = 0; part < nparts; ++part) acc += (double)ds_part[(long long)part * per_part + e];
    img[e] = acc;
}

__global__ __launch_bounds__(256) void afi_swin_bias_table_bwd_kernel(const double* __restrict__ img, int heads, int NP,
                                                                      const int* __restrict__ row_off, const int* __restrict__ pairs, int R,
                                                                      float* __restrict__ dtable) {
    const int id = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (id >= R * heads) return;
    const int r = id / heads, h = id - r * heads;
    const double* src = img + (long long)h * NP * NP;
    double acc = 0.0;
    for (int p = row_off[r] + lane; p < row_off[r + 1]; p += 64) acc += src[pairs[p]];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) dtable[(long long)r * heads + h] += (float)acc;
}

long long afi_swin_bias_table_bwd_ws_floats(int heads, int window) {
    if (heads <= 0 || (window != 7 && window != 12)) return -1;
    const int NP = (window * window + 15) / 16 * 16;
    return 2LL * heads * NP * NP;                                // heads NP NP doubles
}

int afi_swin_bias_table_bwd(const float* ds_part, int nparts, int heads, int window, const int* row_off, const int* pairs, int R, float* dtable,
                            float* ws, long long ws_floats, void* stream) {
    if (!ds_part || !row_off || !pairs || !dtable || nparts <= 0 || heads <= 0 || R <= 0) return AFI_ERR_BAD_ARG;
    if ((window != 7 && window != 12) || ((uintptr_t)ws & 15)) return AFI_ERR_UNSUPPORTED;
    if (!ws || ws_floats < afi_swin_bias_table_bwd_ws_floats(heads, window)) return AFI_ERR_WORKSPACE;
    const int NP = (window * window + 15) / 16 * 16;
    const long long per_part = (long long)heads * NP * NP;
    double* img = (double*)ws;
    hipLaunchKernelGGL(afi_swin_bias_sum_parts_kernel, dim3((unsigned)((per_part + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ds_part, nparts,
                       per_part, img);
    if (hipGetLastError() != hipSuccess) return AFI_ERR_LAUNCH;
    hipLaunchKernelGGL(afi_swin_bias_table_bwd_kernel, dim3(((unsigned)(R * heads) + 3) / 4), dim3(256), 0, (hipStream_t)stream, img, heads, NP,
                       row_off, pairs, R, dtable);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}

// ------------------------------------------------------------------------------------------------ patch gather
// out [N][Ho][Wo][48], channel 16 ci + 4 ky + kx = x[n][ci][4 oy + ky][4 ox + kx] (zero outside H x W): the order of proj.weight.reshape(C, 48).
// Thread = one float4 (the four kx of a (ci, ky)).
__global__ __launch_bounds__(256) void afi_swin_patch_gather_kernel(const float* __restrict__ x, int N, int H, int W, int Ho, int Wo,
                                                                    float* __restrict__ out) {
    const long long total = (long long)N * Ho * Wo * 12;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int g = (int)(i % 12), ci = g >> 2, ky = g & 3;
        const long long pix = i / 12;
        const int ox = (int)(pix % Wo), oy = (int)((pix / Wo) % Ho), n = (int)(pix / ((long long)Wo * Ho));
        const int iy = 4 * oy + ky;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (iy < H) {
            const float* row = x + (((long long)n * 3 + ci) * H + iy) * W;
#pragma unroll
            for (int kx = 0; kx < 4; ++kx)
                if (4 * ox + kx < W) v[kx] = row[4 * ox + kx];
        }
        *(f32x4*)(out + 4 * i) = v;
    }
}

int afi_swin_patch_gather(const float* x, int N, int H, int W, float* out, void* stream) {
    if (!x || !out || N <= 0 || H <= 0 || W <= 0) return AFI_ERR_BAD_ARG;
    if ((uintptr_t)out & 15) return AFI_ERR_UNSUPPORTED;
    const int Ho = (H + 3) / 4, Wo = (W + 3) / 4;
    hipLaunchKernelGGL(afi_swin_patch_gather_kernel, dim3(grid_of((long long)N * Ho * Wo * 12, 256, 16384)), dim3(256), 0, (hipStream_t)stream, x, N,
                       H, W, Ho, Wo, out);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}

// ------------------------------------------------------------------------------------------------ DropPath: out = a + s[n] b
// a, b, out dense [N][per_image] (a NULL: out = s[n] b; out may be a or b).
__global__ __launch_bounds__(256) void afi_swin_scale_add_kernel(const float* a, const float* b, const float* __restrict__ s, long long per4,
                                                                 long long n4, float* out) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const float sn = s[i / per4];
        const f32x4 vb = *(const f32x4*)(b + 4 * i);
        f32x4 va = {0.f, 0.f, 0.f, 0.f};
        if (a) va = *(const f32x4*)(a + 4 * i);
#pragma unroll
        for (int j = 0; j < 4; ++j) va[j] = fmaf(sn, vb[j], va[j]);
        *(f32x4*)(out + 4 * i) = va;
    }
}

int afi_swin_scale_add(const float* a, const float* b, const float* s, int N, long long per_image, float* out, void* stream) {
    if (!b || !s || !out || N <= 0 || per_image <= 0) return AFI_ERR_BAD_ARG;
    if ((per_image & 3) || ((uintptr_t)a & 15) || ((uintptr_t)b & 15) || ((uintptr_t)out & 15)) return AFI_ERR_UNSUPPORTED;
    const long long n4 = (long long)N * (per_image / 4);
    hipLaunchKernelGGL(afi_swin_scale_add_kernel, dim3(grid_of(n4, 256, 16384)), dim3(256), 0, (hipStream_t)stream, a, b, s, per_image / 4, n4, out);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}
