// Internal launchers that cross translation units (not part of the public C-ABI): every function that one .hip file defines and
// another calls is declared HERE and nowhere else, grouped by the file that defines it.  Included by every file that defines or
// calls one of them, so each definition is compiled against the declaration its callers see; default arguments live here only.
#pragma once
#include "afi_common.h"

// ---- igemm.hip
int afi_launch_pix_gemm(const AfiPixGemm& p, int b_rc, hipStream_t st);
int afi_launch_gemm_tn(const float* Q, const float* V, float* dU, int planes, long long rows_per_plane, int M, int N, hipStream_t st, bool deterministic = false);
int afi_launch_gemm_nt(const float* A, const float* B, float* C, int planes, long long rows_per_plane, int N, int K, hipStream_t st);
int afi_launch_split_bf16_tiles(const float* B, void* out, int planes, int N, int K, int split, hipStream_t st);
int afi_launch_gemm_nt_bf16_dma(const float* A, const void* Bsplit, float* C, int planes, long long rows_per_plane, int N, int K, int split, hipStream_t st);
int afi_launch_gemm_tn_bf16(const float* Q, const float* V, float* dU, int planes, long long rows_per_plane, int M, int N, int split, hipStream_t st, bool deterministic = false);
int afi_launch_split_f16_tiles(const float* B, void* out, int planes, int N, int K, hipStream_t st, int wkind = 0);
int afi_f16_image_begin(void* out, hipStream_t st);       // zero-fills the image's header: in front of the weight transform that raises its maximum slot
float* afi_f16_image_wmax(void* out);
long long afi_f16_image_bytes(int planes, int N, int K);
int afi_launch_absmax_planes(const float* X, long long per_plane, int planes, float* out, hipStream_t st);
AfiF16Bound afi_f16_bound(const float* amax, int kind);    // kind: 0 exact per-plane maxima, 1 / 2 F(2x2) / F(4x4) input planes, 3 / 4 F(2x2) / F(4x4) dY planes
int afi_launch_gemm_nt_f16x3(const float* A, const void* Bimg, float* C, int planes, long long rows_per_plane, int N, int K, const AfiF16Bound& ab, hipStream_t st,
                             bool a_pre = false, long long nt256_min_tiles = 512, bool local_sums = false);
int afi_launch_gemm_tn_f16x3(const float* Q, const float* V, float* dU, int planes, long long rows_per_plane, int M, int N, const AfiF16Bound& qb, const AfiF16Bound& vb,
                             hipStream_t st, bool pre = false, bool deterministic = false);
int afi_launch_wgrad_gemm(const AfiWgradGemm& p, hipStream_t st);
int afi_launch_wgrad_gemm_group(const AfiWgradGemm* probs, int n, int wide, hipStream_t st);   // igemm.hip -> smallmap.hip
int afi_launch_wgrad_gemm_group6(const AfiWgradGemm* probs, int n, hipStream_t st);            // the wide group on the bf16 matrix cores (bf16x6)
int afi_launch_pix_gemm_group(const AfiPixGemm* probs, int n, int b_rc, hipStream_t st);
void* afi_prof_open(hipStream_t st, int kind, double flops, long long m, int n, int k);   // the per-launch profiler's bracket for launchers of other files:
void afi_prof_close(void* scope);                                                         // open before the launch, close after it (null: profiling is off)

// ---- smallmap.hip
long long afi_wk6_image_bytes(int Ncols, int Ck, int ntaps, int nKphase);                       // bf16x6 weight images of the small-map kernels
int afi_launch_wk6_images(const AfiWk6ImgJob* jobs, int n, hipStream_t st, const AfiWk6Side* side = nullptr, const AfiWk6ConvT* ct = nullptr);
int afi_launch_pix_gemm_sk(const AfiPixGemm& p, int b_rc, hipStream_t st);                       // these four: called by the launchers of igemm.hip
int afi_launch_pix_gemm_wk_group(const AfiPixGemm* probs, int n, int b_rc, hipStream_t st);
int afi_launch_wgrad_group(const AfiWgradGemm* probs, int n, int wide, hipStream_t st);
int afi_launch_wgrad6_group(const AfiWgradGemm* probs, int n, hipStream_t st);

// ---- frozen1x1.hip
#define AFI_FROZEN1X1_PLAN_SLOTS 12
// what afi_frozen1x1_plan fills (long long each): M, BM, BN, KC, row tiles, column tiles, grid, LDS bytes, byte extent of x, of out (= add), of the image, x dense
enum { AFI_F1_M = 0, AFI_F1_BM, AFI_F1_BN, AFI_F1_KC, AFI_F1_NTM, AFI_F1_NTN, AFI_F1_GRID, AFI_F1_LDS, AFI_F1_XBYTES, AFI_F1_OBYTES, AFI_F1_IBYTES, AFI_F1_XDENSE };

// ---- halfio.hip
int afi_launch_nchw_to_nhwc(const float* in, float* out, int N, int C, int P, hipStream_t st);
int afi_launch_cast_to_f32_nhwc(const void* in, int dt, int N, int C, int H, int W, long long sN, long long sC, long long sH, long long sW, float* out,
                                hipStream_t st);
int afi_launch_cast_from_f32_nhwc(const AfiView& in, int N, int H, int W, int C, void* out, int dt, hipStream_t st);

// ---- elementwise.hip
int afi_launch_colsum_group(const AfiColsumProb* probs, int n, hipStream_t st);
int afi_launch_nhwc_to_nchw(const float* in, float* out, int N, int C, int P, hipStream_t st);
int afi_launch_convT_pack(const float* W, float* Wp, int Cin, int Cout, hipStream_t st);
int afi_launch_convT_unpack_grad(const float* dWp, float* dW, int Cin, int Cout, hipStream_t st);
int afi_launch_rdb_wgrad_unpack(const float* dWp, float* const dw[4], int C, int G, float alpha, hipStream_t st);
int afi_launch_rdb_wgrad_unpack_multi(const float* dWp, long long stride, float* const (*dw)[4], int nblocks, int C, int G, float alpha, hipStream_t st);
int afi_launch_g_bwd_tail(const AfiColsumProb* cs, int n_cs, const float* dWpT, float* dWT, int Cin, int Cout,
                          const float* dWp, long long stride, float* const (*dw)[4], int nblocks, int C, int G, float alpha, hipStream_t st);
int afi_launch_rdb_xpart_pack(const float* const w[4], float* out, int C, int G, hipStream_t st);
int afi_launch_lrelu_slice(AfiView v, int N, int H, int W, int nch, hipStream_t st);
int afi_launch_bn_stats(const float* x, long long P, int C, float* mean, float* invstd, float* var_out, float* running_mean,
                        float* running_var, float* scratch, hipStream_t st, long long* num_batches_tracked = nullptr, float eps = -1.f,
                        float momentum = -1.f, bool fp64 = true);
int afi_launch_bn_stats_from_partials(const double* partial, int rows, long long P, int C, float* mean, float* invstd, float* var_out, float* running_mean,
                                      float* running_var, hipStream_t st, long long* num_batches_tracked = nullptr, float eps = -1.f, float momentum = -1.f);
int afi_launch_view_absmax(AfiView x, int N, int H, int W, int C, float* amax, hipStream_t st);
int afi_launch_bn_apply_lrelu(const float* x, float* y, const float* mean, const float* invstd, const float* gamma, const float* beta,
                              long long P, int C, hipStream_t st, float slope = AFI_LRELU_SLOPE, float* amax = nullptr);
int afi_launch_bn_bwd(const float* g, const float* x, float* dx, const float* mean, const float* invstd, const float* gamma, float* dgamma,
                      float* dbeta, float gscale, long long P, int C, float* scratch, hipStream_t st, const float* mask_beta = nullptr,
                      float slope = AFI_LRELU_SLOPE, float* amax = nullptr);
int afi_launch_colsum_accum(const float* g, long long P, int C, long long ld, float alpha, float* db, float* scratch, hipStream_t st);
int afi_launch_bn_bwd_sums(const float* g, const float* x, const float* mean, const float* invstd, float* dgamma, float* dbeta, float* sums2C, long long P, int C,
                           float* scratch, hipStream_t st);
int afi_launch_bn_bwd_apply(const float* g, const float* x, float* dx, const float* mean, const float* invstd, const float* gamma, const float* sums2C, long long P,
                            long long P_total, int C, hipStream_t st);
int afi_launch_stencil9_sum(const float* d9, int ld, const float* bias, float* out, int N, int H, int W, hipStream_t st);
int afi_launch_stencil9_scatter(const float* dlogit, float* dd9, int ld, int N, int H, int W, hipStream_t st);
extern "C" long long afi_disc_tail_scratch_floats(int C);
int afi_launch_disc_tail_fwd(const float* x, const AfiBnLoad* bn, float slope, const float* w3, float* d9, long long P, int C, hipStream_t st);
int afi_launch_disc_tail_bwd(const float* x, const float* dd9, const AfiBnLoad bn, float slope, const float* w3, float* dx, float* dgamma, float* dbeta, float* dw3,
                             long long P, int C, float* scratch, float* amax, hipStream_t st);
int afi_launch_bce_logits(const float* z, long long n, float target, float lscale, float* loss, float gscale, float* dz, hipStream_t st);
int afi_launch_l1(AfiView a, AfiView b, int N, int h, int w, int C, int Ha, int Wa, float lscale, float* loss, float gscale, float* da,
                  hipStream_t st);
int afi_launch_bilinear2x_fwd(AfiView x, int N, int H, int W, int C, float beta, float* out, hipStream_t st);
int afi_launch_bilinear2x_bwd(const float* dout, int N, int H, int W, int C, float beta, float* dx, hipStream_t st);
int afi_launch_relu_bwd(const float* g, const float* act, float* out, long long n, float s, hipStream_t st);
int afi_launch_dwconv3x3(AfiView x, int N, int H, int W, int C, const float* w, float* out, hipStream_t st);
int afi_launch_maxpool3s2_same(AfiView x, int N, int H, int W, int C, float* out, hipStream_t st);
int afi_launch_fuse_swish(const float* a, const float* b, const float* c, const float* w, float* out, long long n, hipStream_t st);
int afi_launch_sgd(const void* descs_dev, int ntensors, long long max_n, float lr, float mom, float gscale, hipStream_t st);
int afi_launch_scale(float* p, long long n, float s, hipStream_t st);
int afi_launch_sum_accum(const float* v, long long n, float alpha, float* out, hipStream_t st);
int afi_launch_inc_i64(long long* p, hipStream_t st);
int afi_launch_invstd(const float* var, float* invstd, int C, hipStream_t st);

// ---- winograd.hip
#ifndef AFI_STATS_MAX_ROWS
#define AFI_STATS_MAX_ROWS 1024
#endif
int afi_wino_stats_rows(long long T, int C);               // rows of fp64 partials a STATS output transform writes (0: not fused), at most AFI_STATS_MAX_ROWS
int afi_launch_wino_weight(const float* w, float* U, int O, int I, int mode, hipStream_t st, float* wmax = nullptr);
int afi_launch_wino_input(AfiView x, int N, int H, int W, int C, long long Tpad, float* V, hipStream_t st, long long ldo = 0, float* amax = nullptr,
                          const AfiF16Bound* pre = nullptr);
int afi_launch_wino_output(const float* M, long long Tpad, int N, int H, int W, int C, const float* bias, float alpha, AfiView out, AfiView z,
                           hipStream_t st);
int afi_launch_wino_output_epi(const float* M, long long Tpad, const AfiPixGemm& p, hipStream_t st);
int afi_launch_wino_dy(AfiView dy, int N, int H, int W, int C, long long Tpad, float* Q, hipStream_t st, long long ldo = 0, float* amax = nullptr, const AfiF16Bound* pre = nullptr);
int afi_launch_wino_dw(const float* dU, float* dW, int O, int I, float alpha, hipStream_t st);
int afi_launch_wino4_input(AfiView x, int N, int H, int W, int C, long long Tpad, float* V, hipStream_t st, long long ldo = 0, float* amax = nullptr,
                           const AfiF16Bound* pre = nullptr);
int afi_launch_wino4_weight(const float* w, float* U, int O, int I, int mode, hipStream_t st, float* wmax = nullptr);
// f16x3 weight images straight from w (no fp32 U), all of `jobs` in three launches: one fill of wmax_slots[0 .. n), max|w| per job, transform + split
int afi_launch_wino_weight_images(const AfiWinoImgJob* jobs, int n, float* wmax_slots, hipStream_t st);
int afi_launch_wino4_output_epi(const float* M, long long Tpad, const AfiPixGemm& p, hipStream_t st);
int afi_launch_wino4_dy(AfiView dy, int N, int H, int W, int C, long long Tpad, float* Q, hipStream_t st, long long ldo = 0, float* amax = nullptr, const AfiF16Bound* pre = nullptr);
int afi_launch_wino4_dw(const float* dU, float* dW, int O, int I, float alpha, hipStream_t st);
