// Storage-dtype casts at the module boundary (bf16 / fp16 activations under torch.autocast):
//   widen:  bf16 / fp16 / fp32 tensor, NCHW or NHWC with any strides  ->  the dense fp32 [N][H][W][C] the GEMMs read   (exact)
//   narrow: fp32 pixel-major view  ->  dense 2-byte [N][H][W][C] (channels_last), rounded once to nearest even       (csrc/afi_half.h)
// The fp32 NCHW -> NHWC transpose of the detectron2 boundary (afi_nchw_to_nhwc) is the fp32 instance of the widening transpose.
#include "afi_common.h"
#include "afi_launch.h"
#include "afi_half.h"

template <int DT> struct AfiStoreT { typedef unsigned short T; };
template <> struct AfiStoreT<AFI_STORE_F32> { typedef float T; };

template <int DT> __device__ __forceinline__ float afi_load_f32(const typename AfiStoreT<DT>::T* p) {
    if constexpr (DT == AFI_STORE_F32) return *p;
    else return afi_widen1<DT>(*p);
}

// Channel-strided source (NCHW, or any layout whose channel stride is not 1): element (n, c, p) at in[n*sN + c*sC + y*sH + x*sW],
// p = y*W + x.  A block owns 32 channels x 64 pixels: each wave reads one channel row of 64 pixels (128 B of 2-byte, 256 B of fp32 data
// when sW == 1), the LDS tile turns it, and each half-wave writes one pixel's 32 channels (128 B).  Grid (ceil(P/64), ceil(C/32), N).
template <int DT>
__global__ __launch_bounds__(256) void afi_widen_nchw_kernel(const typename AfiStoreT<DT>::T* __restrict__ in, float* __restrict__ out, int C, int H,
                                                              int W, long long sN, long long sC, long long sH, long long sW) {
    __shared__ float tile[32][65];
    const int P = H * W;
    const int n = blockIdx.z, c0 = blockIdx.y * 32, p0 = blockIdx.x * 64;
    const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
    const int p = p0 + lx;
    long long off = 0;
    if (p < P) { const int y = p / W; off = (long long)n * sN + (long long)y * sH + (long long)(p - y * W) * sW; }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int c = c0 + ly + 4 * i;
        if (c < C && p < P) tile[ly + 4 * i][lx] = afi_load_f32<DT>(in + off + (long long)c * sC);
    }
    __syncthreads();
    const int tc = threadIdx.x & 31, tp = threadIdx.x >> 5;
    float* dst = out + (long long)n * P * C;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int pp = p0 + tp + 8 * i, c = c0 + tc;
        if (c < C && pp < P) dst[(long long)pp * C + c] = tile[tc][tp + 8 * i];
    }
}

// Channel-contiguous 2-byte source (channels_last, a crop or a channel slice of one): VEC consecutive channels per thread, 16-byte (VEC 8)
// or 8-byte (VEC 4) loads.  blockIdx.y walks the N*H pixel rows, x the W * C/VEC vectors of a row.
template <int DT, int VEC>
__global__ __launch_bounds__(256) void afi_widen_nhwc_kernel(const unsigned short* __restrict__ in, float* __restrict__ out, int NH, int H, int W, int C,
                                                              long long sN, long long sH, long long sW) {
    const int CV = C / VEC;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= W * CV) return;
    const int x = e / CV, cv = e - x * CV;
    for (int r = blockIdx.y; r < NH; r += gridDim.y) {
        const int n = r / H, y = r - n * H;
        const unsigned short* s = in + (long long)n * sN + (long long)y * sH + (long long)x * sW + cv * VEC;
        float* d = out + ((long long)r * W + x) * C + cv * VEC;
        if constexpr (VEC == 8) {
            typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
            const u32x4 v = *(const u32x4*)s;
            *(f32x4*)d = afi_widen4<DT>(__builtin_bit_cast(afi_u16x4, __builtin_shufflevector(v, v, 0, 1)));
            *(f32x4*)(d + 4) = afi_widen4<DT>(__builtin_bit_cast(afi_u16x4, __builtin_shufflevector(v, v, 2, 3)));
        } else if constexpr (VEC == 4) {
            *(f32x4*)d = afi_widen4<DT>(*(const afi_u16x4*)s);
        } else {
            *d = afi_widen1<DT>(*s);
        }
    }
}

// fp32 pixel-major view -> dense 2-byte [N][H][W][C]: VEC channels per thread (16-byte loads, 8-byte stores for VEC 4; two of each for VEC 8)
template <int DT, int VEC>
__global__ __launch_bounds__(256) void afi_narrow_nhwc_kernel(const float* __restrict__ in, unsigned short* __restrict__ out, int NH, int H, int W, int C,
                                                               long long sN, long long sH, long long sW) {
    const int CV = C / VEC;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= W * CV) return;
    const int x = e / CV, cv = e - x * CV;
    for (int r = blockIdx.y; r < NH; r += gridDim.y) {
        const int n = r / H, y = r - n * H;
        const float* s = in + (long long)n * sN + (long long)y * sH + (long long)x * sW + cv * VEC;
        unsigned short* d = out + ((long long)r * W + x) * C + cv * VEC;
        if constexpr (VEC == 8) {
            typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
            typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
            const u32x2 lo = __builtin_bit_cast(u32x2, afi_narrow4<DT>(*(const f32x4*)s));
            const u32x2 hi = __builtin_bit_cast(u32x2, afi_narrow4<DT>(*(const f32x4*)(s + 4)));
            *(u32x4*)d = u32x4{lo[0], lo[1], hi[0], hi[1]};
        } else if constexpr (VEC == 4) {
            *(afi_u16x4*)d = afi_narrow4<DT>(*(const f32x4*)s);
        } else {
            *d = afi_narrow1<DT>(*s);
        }
    }
}

template <int DT>
static int launch_widen_nchw(const void* in, float* out, int N, int C, int H, int W, long long sN, long long sC, long long sH, long long sW, hipStream_t st) {
    const long long P = (long long)H * W;
    if (P > (1LL << 30) || N > 65535 || afi_cdiv(C, 32) > 65535) return AFI_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(afi_widen_nchw_kernel<DT>, dim3(afi_cdiv(P, 64), afi_cdiv(C, 32), N), dim3(256), 0, st,
                       (const typename AfiStoreT<DT>::T*)in, out, C, H, W, sN, sC, sH, sW);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}

// the widest vector a channel-contiguous view allows: every pixel's first channel `bytes`-aligned and C a multiple of the vector
static int nhwc_vec(const void* p, int esize, int C, long long sN, long long sH, long long sW) {
    for (int v : {8, 4}) {
        const long long b = (long long)v * esize;
        if (C % v == 0 && (uintptr_t)p % b == 0 && sN % v == 0 && sH % v == 0 && sW % v == 0) return v;
    }
    return 1;
}

template <int DT>
static int launch_widen_nhwc(const void* in, float* out, int N, int C, int H, int W, long long sN, long long sH, long long sW, hipStream_t st) {
    const int vec = (uintptr_t)out % 16 == 0 ? nhwc_vec(in, 2, C, sN, sH, sW) : 1;    // (f32x4 stores: dst 16-byte aligned)
    const long long row = (long long)W * (C / vec);
    if (row > (1LL << 30)) return AFI_ERR_UNSUPPORTED;
    const long long NH = (long long)N * H;
    const dim3 grid(afi_cdiv(row, 256), (unsigned)(NH < 65535 ? NH : 65535));
    const unsigned short* s = (const unsigned short*)in;
    if (vec == 8) hipLaunchKernelGGL((afi_widen_nhwc_kernel<DT, 8>), grid, dim3(256), 0, st, s, out, (int)NH, H, W, C, sN, sH, sW);
    else if (vec == 4) hipLaunchKernelGGL((afi_widen_nhwc_kernel<DT, 4>), grid, dim3(256), 0, st, s, out, (int)NH, H, W, C, sN, sH, sW);
    else hipLaunchKernelGGL((afi_widen_nhwc_kernel<DT, 1>), grid, dim3(256), 0, st, s, out, (int)NH, H, W, C, sN, sH, sW);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}

template <int DT>
static int launch_narrow_nhwc(const AfiView& in, void* out, int N, int H, int W, int C, hipStream_t st) {
    const int vec = (uintptr_t)out % 16 == 0 ? nhwc_vec(in.p, 4, C, in.sN, in.sH, in.sW) : 1;
    const long long row = (long long)W * (C / vec);
    if (row > (1LL << 30)) return AFI_ERR_UNSUPPORTED;
    const long long NH = (long long)N * H;
    const dim3 grid(afi_cdiv(row, 256), (unsigned)(NH < 65535 ? NH : 65535));
    unsigned short* d = (unsigned short*)out;
    if (vec == 8) hipLaunchKernelGGL((afi_narrow_nhwc_kernel<DT, 8>), grid, dim3(256), 0, st, in.p, d, (int)NH, H, W, C, in.sN, in.sH, in.sW);
    else if (vec == 4) hipLaunchKernelGGL((afi_narrow_nhwc_kernel<DT, 4>), grid, dim3(256), 0, st, in.p, d, (int)NH, H, W, C, in.sN, in.sH, in.sW);
    else hipLaunchKernelGGL((afi_narrow_nhwc_kernel<DT, 1>), grid, dim3(256), 0, st, in.p, d, (int)NH, H, W, C, in.sN, in.sH, in.sW);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}

int afi_launch_nchw_to_nhwc(const float* in, float* out, int N, int C, int P, hipStream_t st) {
    if (N <= 0 || C <= 0 || P <= 0) return AFI_ERR_BAD_ARG;
    return launch_widen_nchw<AFI_STORE_F32>(in, out, N, C, 1, P, (long long)C * P, P, P, 1, st);
}

int afi_launch_cast_to_f32_nhwc(const void* in, int dt, int N, int C, int H, int W, long long sN, long long sC, long long sH, long long sW, float* out,
                                hipStream_t st) {
    if (!in || !out || N <= 0 || C <= 0 || H <= 0 || W <= 0) return AFI_ERR_BAD_ARG;
    if (dt == AFI_STORE_F32) return launch_widen_nchw<AFI_STORE_F32>(in, out, N, C, H, W, sN, sC, sH, sW, st);
    if (dt != AFI_STORE_BF16 && dt != AFI_STORE_F16) return AFI_ERR_BAD_ARG;
    if (sC == 1 || C == 1)
        return dt == AFI_STORE_BF16 ? launch_widen_nhwc<AFI_STORE_BF16>(in, out, N, C, H, W, sN, sH, sW, st)
                                    : launch_widen_nhwc<AFI_STORE_F16>(in, out, N, C, H, W, sN, sH, sW, st);
    return dt == AFI_STORE_BF16 ? launch_widen_nchw<AFI_STORE_BF16>(in, out, N, C, H, W, sN, sC, sH, sW, st)
                                : launch_widen_nchw<AFI_STORE_F16>(in, out, N, C, H, W, sN, sC, sH, sW, st);
}

int afi_launch_cast_from_f32_nhwc(const AfiView& in, int N, int H, int W, int C, void* out, int dt, hipStream_t st) {
    if (!in.p || !out || N <= 0 || C <= 0 || H <= 0 || W <= 0) return AFI_ERR_BAD_ARG;
    if (dt == AFI_STORE_BF16) return launch_narrow_nhwc<AFI_STORE_BF16>(in, out, N, H, W, C, st);
    if (dt == AFI_STORE_F16) return launch_narrow_nhwc<AFI_STORE_F16>(in, out, N, H, W, C, st);
    return AFI_ERR_BAD_ARG;
}
