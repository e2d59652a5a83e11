// The mask branch of the frozen StandardROIHeads (afigan_amd/roi_heads.py): detectron2 v0.1.1's mask_rcnn_inference and paste_masks_in_image.
// The mask pooler is afi_roi_align at S = 14, the head's 3x3 convs run on the frozen conv dispatch and the deconv (kernel 2, stride 2) is ONE
// afi_conv1x1_fwd over a [4 Cout][Cin] weight, which writes the four output phases of an input pixel side by side: [R][S][S][4][C].
//   afi_roi_mask_probs    the 1x1 predictor on that layout for the row's OWN class only, then the sigmoid.  Shaped like afi_roi_align: lanes run
//                         across channels with 16-byte loads (at C = 256 one output pixel is one coalesced 1 KiB wave load); with fewer than 64
//                         float4 per pixel a wave takes 64 / LW pixels, LW = the power of two >= C / 4.  A wave stays inside one row, so the
//                         class and its weight row are wave-uniform; for C <= 256 the weight row sits in one float4 per lane for the wave's
//                         MASK_GPW pixel groups.  fp32 fmaf per lane in channel order, a fixed xor butterfly, + bias, sigmoid in fp64 rounded once.
//   afi_mask_paste        one block per (detection, band of PASTE_ROWS rows).  The M x M mask sits in LDS inside a one-pixel zero border, so no
//                         tap needs a range test.  A thread owns 16 consecutive columns of every rpp-th row of the band: their x taps and
//                         fractions are computed once per band (fp64 from the fp32 box, operation by operation) and kept in registers; per row it
//                         forms the y tap, the four fp32-rounded weights per pixel, the fmaf sum, the comparison, and writes its 16 result bytes
//                         with one 16-byte store.  Rows of the output start at any byte (W = 1333), so that store is declared unaligned -- the
//                         hardware takes a 16-byte global store at any address -- instead of falling back to byte stores on 15 rows out of 16;
//                         only the last, partial column group of a row is written byte by byte.  Rows and column groups whose pixel centres
//                         are all outside the box store zeros without sampling (the branch is uniform wherever a wave is outside).
// No atomics, no host synchronisation; results are bit-identical from run to run and under hipGraph replay.
#include "../../include/afigan_hip.h"
#include "afi_common.h"

#define MASK_MAX_S 14
#define MASK_GPW 8                  // pixel groups a wave walks with its weight row in registers
#define PASTE_MAX_M 64
#define PASTE_ROWS 32
#define PASTE_COLS 16               // pixels (bytes) per thread and row

// ------------------------------------------------------------------------------------------------ class-selected predictor + sigmoid
// LW: lanes per pixel (power of two, >= C4 when C4 < 64, else 64); G = 64 / LW pixels per wave step; gpr = ceil(4 S S / G) steps per row;
// wpr = ceil(gpr / MASK_GPW) waves per row.
__global__ __launch_bounds__(256) void afi_roi_mask_probs_kernel(const float4* __restrict__ h, const float4* __restrict__ w,
                                                                 const float* __restrict__ bias, const int* __restrict__ classes,
                                                                 const int* __restrict__ counts, int N, int D, int C4, int S, int Km, int LW, int G,
                                                                 int gpr, int wpr, float* __restrict__ probs) {
    const int lane = threadIdx.x & 63;
    const long long wv = (long long)blockIdx.x * 4 + (threadIdx.x >> 6), total = (long long)N * D * wpr;
    if (wv >= total) return;
    const long long row = wv / wpr;
    const int part = (int)(wv - row * wpr), n = (int)(row / D), d = (int)(row - (long long)n * D);
    const int P4 = 4 * S * S;                                   // output pixels of a row in h's order: (y, x, phase)
    const int sub = lane / LW, c0 = lane - sub * LW;
    const int cls = __builtin_amdgcn_readfirstlane(Km == 1 ? 0 : classes[row]);
    const bool live = d < counts[n] && cls >= 0 && cls < Km;    // wave-uniform; a class outside 0 .. Km - 1 reads nothing
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4* wr = w + (long long)(live ? cls : 0) * C4;
    const float bz = live ? bias[cls] : 0.f;
    const float4 wreg = (live && c0 < C4) ? wr[c0] : zero;      // C4 <= 64: the whole weight row, one float4 per lane
    for (int k = 0; k < MASK_GPW; ++k) {
        const int g = part * MASK_GPW + k;
        if (g >= gpr) break;
        const int q = g * G + sub;
        const bool on = sub < G && q < P4;
        float acc = 0.f;
        if (live && on) {
            const float4* hp = h + (row * P4 + q) * C4;
            if (C4 <= 64) {
                if (c0 < C4) {
                    const float4 f = hp[c0];
                    acc = fmaf(wreg.w, f.w, fmaf(wreg.z, f.z, fmaf(wreg.y, f.y, fmaf(wreg.x, f.x, acc))));
                }
            } else {
                for (int c = c0; c < C4; c += 64) {
                    const float4 f = hp[c], u = wr[c];
                    acc = fmaf(u.w, f.w, fmaf(u.z, f.z, fmaf(u.y, f.y, fmaf(u.x, f.x, acc))));
                }
            }
        }
        for (int o = LW >> 1; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
        if (on && c0 == 0) {
            const int pix = q >> 2, ph = q & 3, y = pix / S, x = pix - y * S;
            const float z = acc + bz;
            const float p = live ? (float)(1.0 / (1.0 + exp(-(double)z))) : 0.f;
            probs[row * P4 + (long long)(2 * y + (ph >> 1)) * (2 * S) + 2 * x + (ph & 1)] = p;
        }
    }
}

int afi_roi_mask_probs(const float* h, const float* w, const float* bias, const int* classes, const int* counts, int N, int D, int C, int S, int Km,
                       float* probs, void* stream) {
    if (!h || !w || !bias || !classes || !counts || !probs || N <= 0 || N > 65535 || D <= 0 || C <= 0 || S <= 0 || Km <= 0) return AFI_ERR_BAD_ARG;
    if ((C & 3) || S > MASK_MAX_S || ((uintptr_t)h & 15) || ((uintptr_t)w & 15) || ((uintptr_t)probs & 3) || ((uintptr_t)bias & 3))
        return AFI_ERR_UNSUPPORTED;
    const int C4 = C / 4, P4 = 4 * S * S;
    int LW = 64;
    if (C4 < 64) { LW = 1; while (LW < C4) LW <<= 1; }
    const int G = 64 / LW, gpr = (P4 + G - 1) / G, wpr = (gpr + MASK_GPW - 1) / MASK_GPW;
    const long long blocks = ((long long)N * D * wpr + 3) / 4;
    if (blocks > 0x7fffffffll) return AFI_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(afi_roi_mask_probs_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const float4*)h, (const float4*)w, bias,
                       classes, counts, N, D, C4, S, Km, LW, G, gpr, wpr, probs);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}

// ------------------------------------------------------------------------------------------------ paste
struct __attribute__((packed, aligned(1))) PasteBytes16 { unsigned int a, b, c, d; };      // 16 result bytes stored at any address

// ncg = ceil(W / 16) column groups; cgw = min(ncg, 256) of them side by side in a block; rpp = 256 / cgw rows per pass.
__global__ __launch_bounds__(256) void afi_mask_paste_kernel(const float* __restrict__ probs, const float* __restrict__ boxes, int M, int H, int W,
                                                             int ncg, int cgw, int rpp, float thr, unsigned char* __restrict__ out) {
#pragma clang fp contract(off)                          // the coordinates are the stated fp64 expression, operation by operation; the sum uses fmaf
    extern __shared__ float msk[];                      // [M + 2][M + 2]: the mask inside a zero border (a tap outside 0 .. M - 1 contributes zero)
    const int r = blockIdx.x, tid = threadIdx.x, MP = M + 2;
    const int ya = blockIdx.y * PASTE_ROWS, yb = ya + PASTE_ROWS < H ? ya + PASTE_ROWS : H;
    const float* b = boxes + 4 * (long long)r;
    const double x0 = (double)b[0], y0 = (double)b[1], x1 = (double)b[2], y1 = (double)b[3];
    const double bw = x1 - x0, bh = y1 - y0, dM = (double)M;
    // block-uniform: a box with positive sides (NaN: no) and a row of the band whose centre lies in [y0, y1]
    const bool bandin = bw > 0.0 && bh > 0.0 && (double)yb - 0.5 >= y0 && (double)ya + 0.5 <= y1;
    if (bandin) {
        const float* src = probs + (long long)r * M * M;
        for (int i = tid; i < MP * MP; i += 256) {
            const int yy = i / MP - 1, xx = i - (yy + 1) * MP - 1;
            msk[i] = (yy >= 0 && yy < M && xx >= 0 && xx < M) ? src[yy * M + xx] : 0.f;
        }
        __syncthreads();
    }
    unsigned char* o = out + (long long)r * H * W;
    for (int cgb = 0; cgb < ncg; cgb += cgw) {
        const int rs = tid / cgw, cg = cgb + (tid - rs * cgw);
        if (rs >= rpp || cg >= ncg) continue;
        const int xs = cg * PASTE_COLS, nx = W - xs < PASTE_COLS ? W - xs : PASTE_COLS;
        int ixl[PASTE_COLS];
        double lx[PASTE_COLS];
        unsigned colin = 0;                             // bit j: the centre of column xs + j lies in [x0, x1]
#pragma unroll
        for (int j = 0; j < PASTE_COLS; ++j) {
            ixl[j] = -1;
            lx[j] = 0.0;
            const double xc = (double)(xs + j) + 0.5;
            if (bandin && j < nx && xc >= x0 && xc <= x1) {
                const double gx = (xc - x0) / bw * 2.0 - 1.0;
                const double ix = ((gx + 1.0) * dM - 1.0) / 2.0;
                const double fl = floor(ix);
                int i0 = (int)fl;                       // in -1 .. M - 1 for a centre inside the box (every step above is monotonic)
                i0 = i0 < -1 ? -1 : (i0 > M - 1 ? M - 1 : i0);
                ixl[j] = i0;
                lx[j] = ix - fl;
                colin |= 1u << j;
            }
        }
        for (int y = ya + rs; y < yb; y += rpp) {
            unsigned int pk0 = 0, pk1 = 0, pk2 = 0, pk3 = 0;
            const double yc = (double)y + 0.5;
            if (colin != 0 && yc >= y0 && yc <= y1) {
                const double gy = (yc - y0) / bh * 2.0 - 1.0;
                const double iy = ((gy + 1.0) * dM - 1.0) / 2.0;
                const double fl = floor(iy);
                int i0 = (int)fl;
                i0 = i0 < -1 ? -1 : (i0 > M - 1 ? M - 1 : i0);
                const double ly = iy - fl, hy = 1.0 - ly;
                const float* m0 = msk + (i0 + 1) * MP + 1;
                const float* m1 = m0 + MP;
#pragma unroll
                for (int j = 0; j < PASTE_COLS; ++j) {
                    const double hx = 1.0 - lx[j];
                    const float w00 = (float)(hy * hx), w01 = (float)(hy * lx[j]), w10 = (float)(ly * hx), w11 = (float)(ly * lx[j]);
                    const int xi = ixl[j];
                    float v = fmaf(w00, m0[xi], 0.f);
                    v = fmaf(w01, m0[xi + 1], v);
                    v = fmaf(w10, m1[xi], v);
                    v = fmaf(w11, m1[xi + 1], v);
                    const unsigned bit = (((colin >> j) & 1u) != 0 && v >= thr) ? 1u << (8 * (j & 3)) : 0u;
                    if ((j >> 2) == 0) pk0 |= bit; else if ((j >> 2) == 1) pk1 |= bit; else if ((j >> 2) == 2) pk2 |= bit; else pk3 |= bit;
                }
            }
            unsigned char* p = o + (long long)y * W + xs;
            if (nx == PASTE_COLS) {
                *(PasteBytes16*)p = PasteBytes16{pk0, pk1, pk2, pk3};
            } else {
#pragma unroll
                for (int j = 0; j < PASTE_COLS; ++j) {
                    const unsigned wd = (j >> 2) == 0 ? pk0 : ((j >> 2) == 1 ? pk1 : ((j >> 2) == 2 ? pk2 : pk3));
                    if (j < nx) p[j] = (unsigned char)((wd >> (8 * (j & 3))) & 1u);
                }
            }
        }
    }
}

int afi_mask_paste(const float* probs, const float* boxes, int R, int M, int H, int W, float threshold, unsigned char* out, void* stream) {
    if (R < 0 || M <= 0 || H <= 0 || W <= 0) return AFI_ERR_BAD_ARG;
    if (R == 0) return AFI_OK;
    if (!probs || !boxes || !out) return AFI_ERR_BAD_ARG;
    const int bands = (H + PASTE_ROWS - 1) / PASTE_ROWS;
    if (M > PASTE_MAX_M || bands > 65535 || ((uintptr_t)probs & 3) || ((uintptr_t)boxes & 3)) return AFI_ERR_UNSUPPORTED;
    const int ncg = (W + PASTE_COLS - 1) / PASTE_COLS, cgw = ncg < 256 ? ncg : 256, rpp = 256 / cgw;
    const size_t lds = (size_t)(M + 2) * (M + 2) * sizeof(float);
    hipLaunchKernelGGL(afi_mask_paste_kernel, dim3((unsigned)R, (unsigned)bands), dim3(256), lds, (hipStream_t)stream, probs, boxes, M, H, W, ncg, cgw,
                       rpp, threshold, out);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}
