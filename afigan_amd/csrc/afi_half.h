// 2-byte storage at the module boundary (bf16 / fp16 activations under torch.autocast): conversions shared by the cast kernels
// (csrc/halfio.hip) and the GEMM epilogues.  Both directions are exact or round once, to nearest even, exactly like torch's .to(dtype):
//   fp32 -> bf16: v_cvt_pk_bf16_f32 (NaN stays NaN; the integer rounding trick would turn a NaN with a low payload into inf)
//   fp32 -> fp16: v_cvt_pk_f16_f32 under the default round-to-nearest-even mode (NOT v_cvt_pkrtz_f16_f32, which rounds toward zero);
//                 above 65504 + half an ulp -> inf; fp16 subnormals are kept (the f16 denormal mode is on)
//   bf16 / fp16 -> fp32: exact
#pragma once
#include "afi_common.h"

typedef __bf16 afi_bf16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 afi_f16x4 __attribute__((ext_vector_type(4)));
typedef unsigned short afi_u16x4 __attribute__((ext_vector_type(4)));

template <int DT> __device__ __forceinline__ afi_u16x4 afi_narrow4(f32x4 v) {
    static_assert(DT == AFI_STORE_BF16 || DT == AFI_STORE_F16, "2-byte storage dtypes only");
    if constexpr (DT == AFI_STORE_BF16) return __builtin_bit_cast(afi_u16x4, __builtin_convertvector(v, afi_bf16x4));
    else return __builtin_bit_cast(afi_u16x4, __builtin_convertvector(v, afi_f16x4));
}
template <int DT> __device__ __forceinline__ f32x4 afi_widen4(afi_u16x4 h) {
    static_assert(DT == AFI_STORE_BF16 || DT == AFI_STORE_F16, "2-byte storage dtypes only");
    if constexpr (DT == AFI_STORE_BF16) return __builtin_convertvector(__builtin_bit_cast(afi_bf16x4, h), f32x4);
    else return __builtin_convertvector(__builtin_bit_cast(afi_f16x4, h), f32x4);
}
template <int DT> __device__ __forceinline__ float afi_widen1(unsigned short h) {
    if constexpr (DT == AFI_STORE_BF16) return __builtin_bit_cast(float, (unsigned)h << 16);
    else return (float)__builtin_bit_cast(_Float16, h);
}
template <int DT> __device__ __forceinline__ unsigned short afi_narrow1(float v) {
    if constexpr (DT == AFI_STORE_BF16) return __builtin_bit_cast(unsigned short, (__bf16)v);
    else return __builtin_bit_cast(unsigned short, (_Float16)v);
}

// The store of one float4 of a GEMM output at dst, an address computed inside O as if O held fp32 (AfiPixGemm::o_dtype): fp32 as is,
// or rounded to 2 bytes at the same element index (one 8-byte store).
__device__ __forceinline__ void afi_out_store(const AfiPixGemm& p, float* dst, f32x4 v) {
    if (p.o_dtype == AFI_STORE_F32) { *(f32x4*)dst = v; return; }
    afi_u16x4* d = (afi_u16x4*)((unsigned short*)p.O.p + (dst - p.O.p));
    *d = p.o_dtype == AFI_STORE_BF16 ? afi_narrow4<AFI_STORE_BF16>(v) : afi_narrow4<AFI_STORE_F16>(v);
}
