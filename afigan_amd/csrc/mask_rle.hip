// Pasted masks as COCO run-length starts, straight from the mask probabilities (afigan_amd/roi_heads.py paste_masks_rle): the pixels are
// afi_mask_paste's (mask.hip), expression for expression, but only the pixels inside each box are ever formed and the image-size byte mask is
// never written.  A mask [H][W] is read column-major, j = x H + y; a start is a j whose pixel differs from pixel j - 1 (pixel -1 = 0).
//   afi_mask_rle_bits_kernel   one block per (detection, band of 256 rows, chunk of 256 columns); a block outside the box's pixel extent returns
//                              after reading the box.  The M x M mask sits in LDS inside a one-pixel zero border, a thread owns one row (its y
//                              tap and fraction: one fp64 division per row and block), the chunk's x taps and fractions are computed one per
//                              thread into LDS (one division per column and block).  A wave then walks the columns 64 at a time: every lane
//                              samples its pixel, __ballot makes the 64-row word, the lane of its column keeps it, and after 64
//                              columns the wave stores them with one coalesced 512-byte store: bits[r][word][x], word-major, so that this
//                              store and the column-per-lane reads below are contiguous.
//   afi_mask_rle_starts_kernel one block per detection, a thread per column of the extent (and the column after it, where a run that reaches
//                              the bottom of the last column ends).  The transitions of word k are t = m ^ ((m << 1) | carry), carry = bit 63
//                              of word k - 1, for word 0 the pixel (H - 1, x - 1).  Words and columns outside the extent are zero without
//                              being read.  <false>: the per-column counts to the workspace, the total to nstarts[r].  <true>: the block
//                              scans the per-column counts with a running carry and every thread writes its column's starts, ascending.
// No atomics, no host synchronisation; results are bit-identical from run to run.
#include "../../include/afigan_hip.h"
#include "afi_select.h"

#define RLE_MAX_M 64
#define RLE_TILE 256                // rows per band and columns per chunk of the bits kernel
#define RLE_PASTE_ROWS 32           // afi_mask_paste's band: its bound on H (65535 bands) holds here too

// The pixel extent of a box: columns xa .. xb and rows ya .. yb are exactly those whose centre passes afi_mask_paste's test
// (x0 <= x + 0.5 <= x1: for a finite fp32 x0, x0 - 0.5 is exact in fp64), words wa .. wb of 64 rows.  A box with a non-positive or NaN side
// or a non-finite coordinate, and a box without a pixel centre inside, gives the empty extent (0, -1, 0, -1).
struct RleExtent { int xa, xb, ya, yb, wa, wb; };

__device__ __forceinline__ RleExtent rle_extent(const float* __restrict__ b, int H, int W) {
#pragma clang fp contract(off)
    const double x0 = (double)b[0], y0 = (double)b[1], x1 = (double)b[2], y1 = (double)b[3];
    RleExtent e = {0, -1, 0, -1, 0, -1};
    const bool finite = fabs(x0) <= 3.5e38 && fabs(y0) <= 3.5e38 && fabs(x1) <= 3.5e38 && fabs(y1) <= 3.5e38;      // NaN: no
    if (!(finite && x1 - x0 > 0.0 && y1 - y0 > 0.0)) return e;
    const double dxa = fmin(fmax(ceil(x0 - 0.5), 0.0), (double)W), dxb = fmin(fmax(floor(x1 - 0.5), -1.0), (double)(W - 1));
    const double dya = fmin(fmax(ceil(y0 - 0.5), 0.0), (double)H), dyb = fmin(fmax(floor(y1 - 0.5), -1.0), (double)(H - 1));
    const int xa = (int)dxa, xb = (int)dxb, ya = (int)dya, yb = (int)dyb;
    if (xa > xb || ya > yb) return e;
    e.xa = xa; e.xb = xb; e.ya = ya; e.yb = yb; e.wa = ya >> 6; e.wb = yb >> 6;
    return e;
}

// ------------------------------------------------------------------------------------------------ bits
// grid (R * nchunk, bands); NW = ceil(H / 64) words per column; bits [R][NW][W].
__global__ __launch_bounds__(256) void afi_mask_rle_bits_kernel(const float* __restrict__ probs, const float* __restrict__ boxes, int M, int H, int W,
                                                                int NW, int nchunk, float thr, u64* __restrict__ bits) {
#pragma clang fp contract(off)                          // the coordinates are the stated fp64 expression, operation by operation; the sum uses fmaf
    extern __shared__ float msk[];                      // [M + 2][M + 2]: the mask inside a zero border, as in afi_mask_paste
    __shared__ double s_lx[RLE_TILE], s_hx[RLE_TILE];
    __shared__ int s_ix[RLE_TILE];                      // the x tap + 1 (0 .. M), + 256 when the column's centre lies in [x0, x1]
    const int r = blockIdx.x / nchunk, c0 = (blockIdx.x - r * nchunk) * RLE_TILE, band = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, MP = M + 2;
    const float* b = boxes + 4 * (long long)r;
    const RleExtent e = rle_extent(b, H, W);
    const int xlo = e.xa > c0 ? e.xa : c0, xhi = e.xb < c0 + RLE_TILE - 1 ? e.xb : c0 + RLE_TILE - 1;
    if (xlo > xhi || e.wa > band * 4 + 3 || e.wb < band * 4) return;                    // block-uniform: nothing of the extent here
    const double x0 = (double)b[0], y0 = (double)b[1], x1 = (double)b[2], y1 = (double)b[3];
    const double bw = x1 - x0, bh = y1 - y0, dM = (double)M;
    const float* src = probs + (long long)r * M * M;
    for (int i = tid; i < MP * MP; i += 256) {
        const int yy = i / MP - 1, xx = i - (yy + 1) * MP - 1;
        msk[i] = (yy >= 0 && yy < M && xx >= 0 && xx < M) ? src[yy * M + xx] : 0.f;
    }
    {                                                   // this thread's column of the chunk
        const int x = c0 + tid;
        const double xc = (double)x + 0.5;
        int code = 0;
        double lx = 0.0;
        if (x < W && xc >= x0 && xc <= x1) {
            const double gx = (xc - x0) / bw * 2.0 - 1.0;
            const double ix = ((gx + 1.0) * dM - 1.0) / 2.0;
            const double fl = floor(ix);
            int i0 = (int)fl;                           // in -1 .. M - 1 for a centre inside the box (every step above is monotonic)
            i0 = i0 < -1 ? -1 : (i0 > M - 1 ? M - 1 : i0);
            code = (i0 + 1) | 256;
            lx = ix - fl;
        }
        s_ix[tid] = code;
        s_lx[tid] = lx;
        s_hx[tid] = 1.0 - lx;
    }
    __syncthreads();
    const int k = __builtin_amdgcn_readfirstlane(band * 4 + (tid >> 6));                // this wave's word
    if (k < e.wa || k > e.wb) return;                   // wave-uniform, after the block's only barrier
    const int y = k * 64 + lane;                        // this thread's row
    const double yc = (double)y + 0.5;
    bool rowin = false;
    int iy0 = -1;
    double ly = 0.0;
    if (y < H && yc >= y0 && yc <= y1) {
        const double gy = (yc - y0) / bh * 2.0 - 1.0;
        const double iy = ((gy + 1.0) * dM - 1.0) / 2.0;
        const double fl = floor(iy);
        int i0 = (int)fl;
        i0 = i0 < -1 ? -1 : (i0 > M - 1 ? M - 1 : i0);
        iy0 = i0;
        ly = iy - fl;
        rowin = true;
    }
    const double hy = 1.0 - ly;
    const float* m0 = msk + (iy0 + 1) * MP;             // + the column's tap + 1: rows iy0, iy0 + 1 and columns tap, tap + 1 of the bordered mask
    const float* m1 = m0 + MP;
    u64* o = bits + ((long long)r * NW + k) * W;
    for (int g = 0; g < RLE_TILE / 64; ++g) {
        const int gb = c0 + 64 * g;
        if (gb > xhi || gb + 63 < xlo) continue;
        const int ja = xlo > gb ? xlo - gb : 0, jb = xhi < gb + 63 ? xhi - gb : 63;
        u64 mine = 0;                                   // lane j: the word of column gb + j
        for (int j = ja; j <= jb; ++j) {
            const int t = 64 * g + j, code = s_ix[t], xi = code & 255;
            const double lx = s_lx[t], hx = s_hx[t];
            const float w00 = (float)(hy * hx), w01 = (float)(hy * lx), w10 = (float)(ly * hx), w11 = (float)(ly * lx);
            float v = fmaf(w00, m0[xi], 0.f);
            v = fmaf(w01, m0[xi + 1], v);
            v = fmaf(w10, m1[xi], v);
            v = fmaf(w11, m1[xi + 1], v);
            const u64 word = __ballot(rowin && (code & 256) != 0 && v >= thr);
            if (lane == j) mine = word;
        }
        if (lane >= ja && lane <= jb) o[gb + lane] = mine;
    }
}

// ------------------------------------------------------------------------------------------------ starts: count and emit
// The starts of column x (xa <= x <= xb + 1) in ascending order; returns their number, EMIT writes them to out.
template <bool EMIT>
__device__ __forceinline__ int rle_column(const u64* __restrict__ bits_r, const RleExtent& e, int x, int H, int W, int NW, int* __restrict__ out) {
    const bool incol = x <= e.xb;
    const u64* col = bits_r + x;                        // word k of this column: col[k W]
    const long long j0 = (long long)x * H;
    int n = 0;
    unsigned carry = 0;                                 // pixel (H - 1, x - 1)
    if (x - 1 >= e.xa && x - 1 <= e.xb && e.wb == NW - 1) carry = (unsigned)(col[(long long)(NW - 1) * W - 1] >> ((H - 1) & 63)) & 1u;
    if (e.wa > 0 && carry) {                            // word 0 is zero: the run that reached the bottom of column x - 1 ends here
        if (EMIT) out[n] = (int)j0;
        ++n;
    }
    u64 prev = 0;
    const int kend = e.wb + 1 < NW - 1 ? e.wb + 1 : NW - 1;
    for (int k = e.wa; k <= kend; ++k) {
        const u64 m = (incol && k <= e.wb) ? col[(long long)k * W] : 0ull;
        const u64 c = k == 0 ? (u64)carry : prev >> 63;
        u64 t = m ^ ((m << 1) | c);
        if (k == NW - 1 && (H & 63)) t &= (1ull << (H & 63)) - 1ull;
        if (EMIT) {
            u64 q = t;
            int i = n;
            while (q) {
                out[i++] = (int)(j0 + 64 * k + __builtin_ctzll(q));
                q &= q - 1ull;
            }
        }
        n += __popcll(t);
        prev = m;
    }
    return n;
}

// colcnt [R][W]; <false>: nstarts [R] written; <true>: offsets [R] read, starts written.
template <bool EMIT>
__global__ __launch_bounds__(256) void afi_mask_rle_starts_kernel(const float* __restrict__ boxes, int H, int W, int NW, const u64* __restrict__ bits,
                                                                  int* __restrict__ colcnt, int* __restrict__ nstarts,
                                                                  const long long* __restrict__ offsets, int* __restrict__ starts) {
    __shared__ int wtot[16];
    const int r = blockIdx.x, tid = threadIdx.x;
    const RleExtent e = rle_extent(boxes + 4 * (long long)r, H, W);
    const u64* bits_r = bits + (long long)r * NW * W;
    int* cc = colcnt + (long long)r * W;
    const int xend = e.xb + 1 < W - 1 ? e.xb + 1 : W - 1;              // the empty extent: column 0 alone, which reads nothing and counts zero
    long long run = EMIT ? offsets[r] : 0;
    for (int xb = e.xa; xb <= xend; xb += 256) {                        // block-uniform trip count
        const int x = xb + tid;
        const bool on = x <= xend;
        int v = 0;
        if (on) v = EMIT ? cc[x] : rle_column<false>(bits_r, e, x, H, W, NW, nullptr);
        if (!EMIT && on) cc[x] = v;
        int total;
        const int inc = rpn_block_scan(v, wtot, &total);
        if (EMIT && on && v) rle_column<true>(bits_r, e, x, H, W, NW, starts + (run + inc - v));
        run += total;
    }
    if (!EMIT && tid == 0) nstarts[r] = (int)run;
}

// ------------------------------------------------------------------------------------------------ entry points
static bool rle_shape_ok(int H, int W) {
    return (long long)H * W < 0x80000000ll && (H + RLE_PASTE_ROWS - 1) / RLE_PASTE_ROWS <= 65535;
}

long long afi_mask_rle_ws_bytes(int R, int H, int W) {
    if (R < 0 || H <= 0 || W <= 0 || !rle_shape_ok(H, W)) return -1;
    const long long NW = (H + 63) / 64;
    return (long long)R * NW * W * 8 + (((long long)R * W * 4 + 7) & ~7ll);
}

int afi_mask_rle_count(const float* probs, const float* boxes, int R, int M, int H, int W, float threshold, void* ws, long long ws_bytes,
                       int* nstarts, void* stream) {
    if (R < 0 || M <= 0 || H <= 0 || W <= 0) return AFI_ERR_BAD_ARG;
    if (R == 0) return AFI_OK;
    if (!probs || !boxes || !ws || !nstarts) return AFI_ERR_BAD_ARG;
    const int nchunk = (W + RLE_TILE - 1) / RLE_TILE, bands = (H + RLE_TILE - 1) / RLE_TILE, NW = (H + 63) / 64;
    if (M > RLE_MAX_M || !rle_shape_ok(H, W) || (long long)R * nchunk > 0x7fffffffll || ((uintptr_t)probs & 3) || ((uintptr_t)boxes & 3) ||
        ((uintptr_t)ws & 7) || ((uintptr_t)nstarts & 3))
        return AFI_ERR_UNSUPPORTED;
    if (ws_bytes < afi_mask_rle_ws_bytes(R, H, W)) return AFI_ERR_BAD_ARG;
    u64* bits = (u64*)ws;
    int* colcnt = (int*)(bits + (long long)R * NW * W);
    const size_t lds = (size_t)(M + 2) * (M + 2) * sizeof(float);
    hipLaunchKernelGGL(afi_mask_rle_bits_kernel, dim3((unsigned)(R * nchunk), (unsigned)bands), dim3(256), lds, (hipStream_t)stream, probs, boxes, M,
                       H, W, NW, nchunk, threshold, bits);
    hipLaunchKernelGGL(afi_mask_rle_starts_kernel<false>, dim3((unsigned)R), dim3(256), 0, (hipStream_t)stream, boxes, H, W, NW, (const u64*)bits,
                       colcnt, nstarts, (const long long*)nullptr, (int*)nullptr);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}

int afi_mask_rle_emit(const float* boxes, int R, int H, int W, const void* ws, long long ws_bytes, const long long* offsets, int* starts,
                      void* stream) {
    if (R < 0 || H <= 0 || W <= 0) return AFI_ERR_BAD_ARG;
    if (R == 0) return AFI_OK;
    if (!boxes || !ws || !offsets || !starts) return AFI_ERR_BAD_ARG;
    if (!rle_shape_ok(H, W) || ((uintptr_t)boxes & 3) || ((uintptr_t)ws & 7) || ((uintptr_t)offsets & 7) || ((uintptr_t)starts & 3))
        return AFI_ERR_UNSUPPORTED;
    if (ws_bytes < afi_mask_rle_ws_bytes(R, H, W)) return AFI_ERR_BAD_ARG;
    const int NW = (H + 63) / 64;
    const u64* bits = (const u64*)ws;
    int* colcnt = (int*)(bits + (long long)R * NW * W);                // read only here
    hipLaunchKernelGGL(afi_mask_rle_starts_kernel<true>, dim3((unsigned)R), dim3(256), 0, (hipStream_t)stream, boxes, H, W, NW, bits, colcnt,
                       (int*)nullptr, offsets, starts);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}
