/*
 * afigan_hip.h -- C-ABI of the MI355X-native AFI-GAN hot path (libafigan_hip.so, gfx950).
 *
 * The reference (inhavl-shlee/AFI-GAN) is pure Python: its "plugin API" for this path is two nn.Module
 * classes,  Generator (afigan/modeling/feat_interpol/generator_rdb.py:73-130)  and
 * Discriminator (afigan/modeling/feat_interpol/feature_patch_discriminator.py:16-55),  plus the loss /
 * optimizer calls of the stage-1 loop (afigan/engine/stage1_trainer.py:305-443).  It has no FFI of its own,
 * so this header defines the boundary a binding for that path needs: plain pointers, sizes and a HIP stream;
 * no torch types; every function returns an int status (AFI_OK == 0) and never throws or allocates.
 * The Python binding a maintainer would add (ctypes) is shown in INTEGRATION.md and shipped in
 * afigan_amd/_lib.py.  That binding READS this file at import: argument and return types come from the
 * prototypes below, option / dtype / pool numbers from the #defines.  A new entry point needs a prototype
 * here, a definition under afigan_amd/csrc and a wrapper in afigan_amd/ops.py -- no table anywhere else.
 * Keep to the types the binding knows (int, long long, float, double, afi_view_t by value, pointers, named
 * parameters): anything else is refused at import, never guessed.
 *
 * Conventions
 *   - Activations are PIXEL-MAJOR ("NHWC"): element (n, y, x, c) of a view lives at
 *     p[n*sN + y*sH + x*sW + c]; strides are in floats, the channel stride is 1.  A torch tensor in
 *     torch.channels_last memory format is exactly this (zero copy); cropped views
 *     (stage1_trainer.py:437-443) and channel slices of wider buffers are expressed through p / strides.
 *   - 3x3 weights are  [Cout][3][3][Cin]  (the physical layout of a [Cout,Cin,3,3] tensor in channels_last
 *     format, so the reference's state_dict shapes are unchanged); the ConvTranspose2d weight stays in torch's
 *     [Cin][Cout][6][6] layout.  All data is fp32 in memory.  Matrix math: the Winograd-domain GEMMs of the big 3x3 convs in the context's arithmetic
 *     (afi_ctx_set_compute_dtype: by default fp32 products formed exactly on the bf16 matrix cores), every other GEMM on v_mfma_f32_32x32x2_f32 (exact f32).
 *   - Channel counts must be multiples of 4 (float4 granularity); spatial sizes are arbitrary.
 *   - "accumulate" outputs (all gradients w.r.t. parameters) are += targets: zero them first, like
 *     optimizer.zero_grad() at stage1_trainer.py:374/426.
 *   - `stream` is a hipStream_t passed as void* (NULL = the legacy default stream).
 *   - `ctx` (first argument of the convolution and whole-network entry points) is the caller's afi_ctx_t or NULL, see below.
 */
#ifndef AFIGAN_HIP_H
#define AFIGAN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AFI_OK 0
#define AFI_ERR_BAD_ARG 1
#define AFI_ERR_UNSUPPORTED 2
#define AFI_ERR_LAUNCH 3
#define AFI_ERR_WORKSPACE 4

#define AFI_MAX_RDB 8

typedef struct afi_view {
    float* p;
    long long sN, sH, sW;
} afi_view_t;

int afi_abi_version(void);
const char* afi_status_string(int status);

/* ------------------------------------------------------------------ caller-owned context
 * Every piece of library state that outlives one call lives in an afi_ctx_t the caller creates, passes to the entry points that can
 * use it, and destroys: the split-K scratch of the per-op calls, the cache of transformed / packed weights, the transform-domain
 * weight-gradient accumulator, and the side stream the backward passes fork their weight gradients onto.  NOTHING is process-global
 * (the reference's modules keep their state per nn.Module instance; SURVEY 8b: "thread-safe per stream; no global mutable state").
 *   - One context serves ONE stream at a time on the device that was current when it was created (calls on another device return
 *     AFI_ERR_BAD_ARG); two engines / threads use two contexts and share nothing.
 *   - ctx may be NULL in every entry point: no scratch, no caches, no side stream (everything on `stream`, every transform per call).
 *   - The library never allocates device memory: the three buffers are the caller's and must stay alive and unchanged in meaning while
 *     registered (floats == 0 unregisters).  The side stream and its events are created on first use and released by afi_ctx_destroy. */
typedef struct afi_ctx afi_ctx_t;
/* sha256 (hex) of the sources the binary was compiled from -- every *.hip / *.h under afigan_amd/csrc and this header, in sorted order of
 * their names -- written into the build by __graft_entry__.build(); "unknown" for a build that bypassed it.  afigan_amd/_lib.py recomputes it
 * from the tree and refuses a library that was built from other sources: "which binary ran" has one answer. */
const char* afi_build_id(void);
int afi_ctx_create(afi_ctx_t** out);
int afi_ctx_destroy(afi_ctx_t* ctx);                       /* refused (AFI_ERR_BAD_ARG) while weight-gradient sums are pending */
/* Scratch for the PER-OP convolution entry points (afi_conv3x3_*, afi_conv1x1_*, afi_conv3x3s2_*, afi_convT6s2_*): with it, mid-size maps
 * (< 6 tiles of 128x128 per CU) run split-K with a deterministic second pass.  256 MB covers every shape that is split.  (The whole-net
 * entry points carve their split-K scratch out of the workspace they are given.) */
int afi_ctx_set_op_scratch(afi_ctx_t* ctx, float* scratch, long long floats);
/* Arithmetic of the Winograd-domain GEMMs issued under this context -- every 3x3 / stride-1 convolution with >= 128 channels on both
 * sides and >= 1024 pixels, forward, data gradient and weight gradient, i.e. >= 95 % of a stage-1 step's FLOPs.  Tensors, transforms,
 * epilogues, accumulators and every other kernel are fp32 under every setting; the settings differ in how a product of two fp32
 * operands is formed on the matrix cores (gfx950 runs fp32 MFMAs at 1/16 of its bf16 MFMA rate, and has no xf32).  Measured max-norm
 * error of the batched GEMM against fp64 on the same operands (tools/gemm_nt_dtype.py; tolerances asserted in tests/test_gpu_bf16.py):
 *   AFI_DTYPE_BF16X6  (default) each operand is split EXACTLY into three bf16, x = hi + mid + lo (3 x 8 = all 24 mantissa bits; the
 *                     residuals x - hi and x - hi - mid are exact in fp32), and the six partial products of order >= 2^-16
 *                     (hi*hi, hi*mid, mid*hi, mid*mid, hi*lo, lo*hi) are accumulated smallest first in fp32 by the bf16 MFMA (16x16x32 / 32x32x16);
 *                     a bf16 x bf16 product is exact in fp32, and what is dropped (mid*lo, lo*mid, lo*lo <= 2^-23 of a product) is the
 *                     size of fp32's own rounding of that product.  Error 0.5e-6 .. 1.1e-6 -- at or below the fp32 MFMA's on every shape
 *                     measured -- at 1.5x its speed.  fp32-grade: every parity test of this repo runs on it at the fp32 tolerances.
 *   AFI_DTYPE_F16X3   each operand is scaled by a power of two (per operand and Winograd plane, exact) and split into TWO fp16 pieces,
 *                     x s = hi + lo + r with |r| <= 2^-23 |x s| (round to nearest; 11 + 11 significant bits, the residual x s - hi exact in
 *                     fp32); the three products hi*hi, hi*lo, lo*hi are accumulated smallest first in fp32 by the f16 MFMA (same rate as
 *                     the bf16 one), the dropped lo*lo is <= 2^-22 of a product with random sign, and the accumulator is scaled back by
 *                     the exact inverse in the epilogue.  Half the matrix-core work of BF16X6.  The scale needs the operand's largest
 *                     magnitude before the GEMM starts: the Winograd transforms that write the planes compute the largest magnitude of
 *                     the tensor they read as a by-product, and every plane is bounded by a constant times it (csrc/afi_gemm_f16.h);
 *                     elements more than ~2^18 below the plane's bound lose RELATIVE precision (their absolute error stays <= 2^-40 of
 *                     the bound), which a max-norm comparison with fp32 does not see and a dot product does not feel.  fp32-grade on
 *                     the operands of tests/test_gpu_bf16.py::test_f16x3_is_fp32_grade_on_hard_operands.
 *   AFI_DTYPE_F32     fp32 MFMA (v_mfma_f32_32x32x2_f32, bit-identical to an fmaf chain).  Error 1.0e-6 .. 1.3e-6.
 *   AFI_DTYPE_BF16X3  x = hi + lo (16 mantissa bits), three MFMAs (hi*hi + hi*lo + lo*hi).  Error 4.5e-6; conv outputs within 2e-4,
 *                     network outputs / input gradients within 1e-3, weight gradients within 1e-2 (L2; LeakyReLU-mask flips).  Opt-in.
 *   AFI_DTYPE_BF16    operands rounded to bf16 (8 bits), one MFMA; every convolution on F(2x2,3x3) tiles (the F(4x4) transforms do not
 *                     survive 8-bit operands: 3 % error).  Error 2.5e-3; conv outputs within 2e-2, networks 5e-2 / 1e-1.  Opt-in:
 *                     the reference has no reduced-precision mode (SOLVER.AMP is never read, defaults.py:82).
 * What follows the setting: the three batched GEMMs of a Winograd convolution -- forward (NT), data gradient (NT on the flipped weights)
 * and weight gradient (TN) -- so a backward pass runs in the arithmetic its forward ran in (the autograd wrappers carry the forward's context
 * into backward).  What never does: the direct implicit-GEMM kernels (1x1 and lateral convs, stride-2 and transposed convs, ragged / small
 * maps, the small-map grouped kernels) and their weight-gradient GEMMs multiply on v_mfma_f32_32x32x2_f32 under every setting.
 * Refused while weight-gradient sums are pending.  No environment variable changes the default. */
#define AFI_DTYPE_F32 0
#define AFI_DTYPE_BF16 1
#define AFI_DTYPE_F16X3 2
#define AFI_DTYPE_BF16X3 3
#define AFI_DTYPE_BF16X6 6
#define AFI_DTYPE_DEFAULT AFI_DTYPE_F16X3
int afi_ctx_set_compute_dtype(afi_ctx_t* ctx, int dtype);
int afi_ctx_get_compute_dtype(const afi_ctx_t* ctx);
/* Algorithm options of a context.  The library reads NO environment variable: every choice that changes numerics or scheduling is made
 * here, per context, and may be changed between calls (refused while weight-gradient sums are pending).  ctx == NULL reads the default. */
#define AFI_OPT_WINOGRAD 0                    /* 1 (default): 3x3 / stride-1 convs with >= 128 channels on both sides run in Winograd form from the pixel
                                                 thresholds below; 0: direct implicit GEMM on the fp32 MFMA everywhere */
#define AFI_OPT_WINOGRAD_F4_BACKWARD 1        /* 1 (default): F(4x4,3x3) / F(3x3,4x4) for data and weight gradients and for forwards no backward follows,
                                                 from 8192 pixels; 0: F(2x2,3x3) everywhere */
#define AFI_OPT_WINOGRAD_F4_FORWARD 2         /* the discriminator forwards a backward follows (their conv outputs decide LeakyReLU masks), per block:
                                                 bit n + 1 puts block n on F(4x4) (2: block 0, 4: block 1, 8: block 2; sums combine); 1: every block;
                                                 0: F(2x2) everywhere.  Default 12 (blocks 1 and 2, with AFI_OPT_F16_LOCAL_SUMS = 12): the largest block set whose gradient
                                                 deviation from fp64 stays below torch's own fp32 ops on the same inputs at P2 and at P3
                                                 (profiles/r06/dflip_p2_*_6seeds_local_sums.txt, dflip_p3_*: D fwd+bwd, relative L2 of dx / worst parameter gradient, means
                                                 over six seeds; P3 | P2): torch fp32 1.15e-3 / 1.54e-3 | 1.21e-3 / 1.54e-3; = 0: 0.79e-3 / 1.06e-3 | 0.88e-3 / 1.18e-3;
                                                 = 8: 0.97e-3 / 1.31e-3 | 1.14e-3 / 1.51e-3; = 12 in the plain summation order (round 5's default): 1.27e-3 / 1.73e-3 |
                                                 1.45e-3 / 1.91e-3; = 12 with the local sums: 0.88e-3 / 1.26e-3 | 1.04e-3 / 1.33e-3; = 1 with them: 1.32e-3 / 1.79e-3 |
                                                 1.40e-3 / 1.76e-3.  tests/test_gpu_d_parity.py holds the default to that bar.
                                                 Bit 16: the interpolator's own forwards too (off: 15x the deviation on its worst parameter gradient for 1 ms) */
#define AFI_OPT_BN_STATS_FP64 3               /* 1 (default): BatchNorm batch statistics accumulated in fp64 (torch's CPU accumulation type).
                                               * 0: the fp32 one-pass form shifted by row 0, which loses the order of 1 % of the variance when row 0
                                               * is an outlier of 1e3 standard deviations, as the shift then removes nothing (emulated in fp32 on
                                               * the CPU in the kernels' summation order: 0.3 % at 8400 rows, 3.6 % at 134400). */
#define AFI_OPT_D_WINOGRAD_MIN_PIXELS 4       /* 1024: discriminator calls of fewer pixels stay direct (values below 1024 act as 1024) */
#define AFI_OPT_G_WINOGRAD_MIN_PIXELS 5       /* 2048: the same for a convolution of the interpolator */
#define AFI_OPT_G_SMALLMAP_MAX_PIXELS 6       /* 2048: below, the dense blocks run in column-batched form (5 grouped launches per block); 0: never */
#define AFI_OPT_G_GROUPED_WGRAD_MAX_PIXELS 7  /* 3000: up to here all weight / bias gradients of a backward pass run as three grouped launches; 0: per layer */
#define AFI_OPT_G_BATCH_GROWTH_GRADS 8         /* 1 (default): above G_GROUPED_WGRAD_MAX_PIXELS the four growth convs of a dense block are batched where they share
                                               * an operand: what they take from the block input is ONE conv C -> 4G on packed weights [4G][3][3][C] (forward) and ONE
                                               * data gradient 4G -> C (backward), their weight gradients ONE 4G-row GEMM (packed, then unpacked) -- all Winograd-
                                               * eligible at the reference's widths; 0: four G-column / G-row GEMMs per block, as generator_rdb.py:64-71 reads */
#define AFI_OPT_G_SMALLMAP6_MAX_PIXELS 9      /* 4096: under AFI_DTYPE_BF16X6 (and channel counts that are multiples of 32) interpolator calls of up to this many
                                               * low-res pixels run the small-map schedule -- column-batched dense blocks, grouped weight gradients, every conv on the
                                               * bf16x6 small-map kernels with pre-split weight images (csrc/smallmap.hip) -- whatever options 5..7 say; 0: options 5..7 alone */
#define AFI_OPT_DETERMINISTIC 10              /* 0 (default): weight-gradient GEMMs whose pixel range is split over blocks add their partial tiles by fp32 atomics
                                               * (summation order varies run to run: results agree to ~1e-6, not bit for bit).  1: no weight gradient is split
                                               * over blocks -- the Winograd TN GEMM and the direct weight-gradient kernel run one block per tile over the whole
                                               * pixel range, the interpolator's small-map backward takes the per-layer launches instead of the grouped
                                               * stream-K ones, bias sums take the two-stage fixed-order reduction -- so that two runs from the same state produce
                                               * the same bits (a resumed run continues bit for bit: tests/test_gpu_stage1.py).  Slower: for reproducing, not for speed. */
#define AFI_OPT_F16_PRESPLIT 11               /* 1 (default): under AFI_DTYPE_F16X3, a Winograd transform whose source tensor's largest magnitude is known before it
                                               * runs (the discriminator's activations and gradients: published by the BatchNorm passes that write them) writes
                                               * its planes already split into the two fp16 pieces and the GEMM stages them by DMA alone.  0: every plane is
                                               * written in fp32 and split when the GEMM reads its fragments (same results; stage-1 step 86.6 against 84.4 ms).
                                               * Bit 1 (value 3: planes pre-split as under 1) is the A/B switch of the WEIGHT images: clear (the default), the pre-split
                                               * weight image of a tile-aligned Winograd conv (forward or data gradient) is built straight from w by the grouped builder
                                               * of csrc/winograd.hip -- one fill of the maxima slots, one pass over the raw weights for max|w|, one pass that
                                               * transforms in registers and writes the fp16 pieces and the image header: three launches for ALL the images a
                                               * whole-net call misses (the discriminator's and the interpolator's passes list theirs at entry; a single conv is a
                                               * table of one), and the fp32 planes U are neither written nor read; set, every image takes a header fill, the fp32
                                               * weight transform and the split that reads it back.  Same bytes either way (tests/test_gpu_weight_images.py) */
#define AFI_OPT_F16_NT256_MIN_TILES 12        /* 512: the f16x3 NT GEMM takes its 256 x 256 tile (sixteen waves per block, half the operand bytes per product)
                                               * from this many tiles on (and 256-column multiples); 0: never (the 128 x 128 tile everywhere) */
#define AFI_OPT_F16_LOCAL_SUMS 13             /* under AFI_DTYPE_F16X3, which of the discriminator's forward convs that a backward follows (training == 1: their rounding
                                               * decides LeakyReLU masks) sum the three products of every k-step in a fresh fragment and add that fragment to the
                                               * accumulator with ONE fp32 addition, instead of three accumulating MFMAs: bit n + 1 = block n, 1 = every block, 0 = none.
                                               * Same products, fewer roundings of the large accumulator (an fp32 accumulate rounds at the accumulator's magnitude,
                                               * whatever the addend).  Pre-split planes and 256-column multiples only (blocks 1 and 2 at the reference's widths; other
                                               * shapes keep the plain order).  Default and measurements: DESIGN.md 0 / 4b */
#define AFI_OPT_D_FUSE_TAIL 14                /* 1 (default): the discriminator's last block and last conv (F3 -> 1, F3 <= 1024, F3 % 16 == 0) run fused -- the last conv reads the
                                               * block's saved conv output through its BatchNorm affine + LeakyReLU (the activation y[2] is never written:
                                               * afi_discriminator_saved_activations), and the block's BatchNorm backward GENERATES the gradient with respect to that
                                               * activation from the nine logit gradients of each pixel instead of reading it, taking the last conv's weight gradient
                                               * along: at 2 x 200 x 336 x 1024, 1.1 GB less traffic per forward and 2.2 GB less per backward.  Same decisions of
                                               * the LeakyReLU masks (the pinned affine), sums in another order.  0: the separate passes of rounds 1-5 */
#define AFI_OPT_COUNT 15
int afi_ctx_set_option(afi_ctx_t* ctx, int option, long long value);
long long afi_ctx_get_option(const afi_ctx_t* ctx, int option);
/* The batched "NT" GEMM those convolutions run on, for tests and micro-benchmarks:  C[g][m][n] = sum_k A[g][m][k] * B[g][n][k] over
 * `planes` groups; rows_per_plane % 128 == 0, N % 128 == 0, K % 32 == 0 (else AFI_ERR_UNSUPPORTED); fp32 in memory for every dtype.
 * Under the bf16 settings the B operand (inside the library: the transformed weights, shared by every row tile of a plane) is first split
 * into bf16 parts in the order the kernel's LDS-DMA stages it; `scratch` (afi_gemm_nt_scratch_bytes; 0 for fp32) receives that image.
 * The library never allocates: too little scratch is AFI_ERR_WORKSPACE. */
long long afi_gemm_nt_scratch_bytes(int planes, int N, int K, int dtype);
int afi_gemm_nt(const float* A, const float* B, float* C, int planes, long long rows_per_plane, int N, int K, int dtype, void* scratch,
                long long scratch_bytes, void* stream);
/* ... and the weight-gradient form  dU[g][m][n] += sum_k Q[g][k][m] * V[g][k][n]  (both operands k-slow; rows_per_plane = K per plane,
 * % 32 == 0; M % 128 == 0, N % 128 == 0).  Split-K with fp32 atomics: the summation order varies run to run.  `scratch`
 * (afi_gemm_tn_scratch_bytes: 512 under AFI_DTYPE_F16X3 -- the per-plane maxima of both operands --, 0 otherwise; may be NULL then). */
long long afi_gemm_tn_scratch_bytes(int planes, int dtype);
int afi_gemm_tn(const float* Q, const float* V, float* dU, int planes, long long rows_per_plane, int M, int N, int dtype, void* scratch,
                long long scratch_bytes, void* stream);
/* Cache of the Winograd-transformed (and packed conv-transpose) weights.  Within one phase of a training step the same weights serve up
 * to ten calls (stage1_trainer.py:336-433: five levels x real / fake); each (weight pointer, tiling, direction) is transformed once and
 * re-used until afi_ctx_wino_weight_cache_invalidate() -- which the caller MUST issue whenever weight VALUES change (optimizer step,
 * load, broadcast); the weight MEMORY must stay allocated while entries exist (a freed-and-reused address would alias another weight).
 * Registering also invalidates.  140 M floats hold every transform of the reference's G and D. */
int afi_ctx_set_wino_weight_cache(afi_ctx_t* ctx, float* buf, long long floats);
int afi_ctx_wino_weight_cache_invalidate(afi_ctx_t* ctx);
/* Accumulator for the Winograd weight gradients.  While one is registered, every Winograd weight-gradient call adds its transform-domain
 * sum dU into a slot keyed by its dW target instead of zero-filling and transforming per call; the caller MUST call
 * afi_ctx_wino_wgrad_flush(ctx, stream) -- dW += alpha * A'^T dU A' for every slot, then the slots are released -- before it reads the
 * gradients (all-reduce, optimizer step), on a stream ordered after the calls that accumulated; after a failed phase
 * afi_ctx_wino_wgrad_discard drops the pending sums instead.  (Un)registering with sums pending is refused.  100 M floats hold every
 * slot of the reference's G and D. */
int afi_ctx_set_wino_wgrad_accum(afi_ctx_t* ctx, float* buf, long long floats);
int afi_ctx_wino_wgrad_flush(afi_ctx_t* ctx, void* stream);
int afi_ctx_wino_wgrad_discard(afi_ctx_t* ctx);

/* ------------------------------------------------------------------ whole-network entry points */

/* Parameters of Generator.Generators[0]  (generator_rdb.py:87-108; state_dict names in SURVEY.md 8b). */
typedef struct afi_gen_params {
    int C;                  /* in_channels (256) */
    int G;                  /* growth_rate (32) */
    int n_rdb;              /* n_residual_dense_blocks (3 in every caller) */
    float residual_scale;   /* 0.2 */
    float* w0; float* b0;                    /* Generators.0.0.0.{weight,bias}                       */
    float* rdb_w[AFI_MAX_RDB][5];            /* Generators.0.1.RDBs.r.conv{1..4}.0.weight, conv5.weight */
    float* w7; float* b7;                    /* Generators.0.2.0.{weight,bias}                       */
    float* wT; float* bT;                    /* Generators.0.3.0.{weight [Cin][Cout][6][6], bias}    */
    float* w9; float* b9;                    /* Generators.0.4.0.{weight,bias}                       */
} afi_gen_params_t;

/* floats of workspace needed by afi_generator_fwd (saved activations + packed conv-transpose weight) */
long long afi_generator_fwd_ws_floats(int C, int G, int n_rdb, int N, int H, int W);
/* floats of scratch needed by afi_generator_bwd */
long long afi_generator_bwd_ws_floats(int C, int G, int n_rdb, int N, int H, int W);

/* out[N,2H,2W,C] = bilinear_x2(x) + Generators[0](x)      (Generator.forward, generator_rdb.py:123-130) */
int afi_generator_fwd(afi_ctx_t* ctx, const afi_gen_params_t* prm, afi_view_t x, int N, int H, int W, afi_view_t out,
                      float* ws, long long ws_floats, void* stream);
/* Backward of the above.  `ws` is the forward workspace (unchanged since the forward), `dout` a DENSE
 * [N,2H,2W,C] gradient, `grads` the += targets laid out like the params (any pointer may be NULL to skip),
 * `dx` a DENSE [N,H,W,C] buffer or NULL when the input needs no gradient (stage 1: lr features are detached). */
int afi_generator_bwd(afi_ctx_t* ctx, const afi_gen_params_t* prm, const afi_gen_params_t* grads, afi_view_t x, int N, int H, int W,
                      const float* ws, const float* dout, float* dx, float* scratch, long long scratch_floats, void* stream);

/* Storage dtype of a tensor at the module boundary (bf16 / fp16 activations under torch.autocast).  It is not an arithmetic setting:
 * every kernel computes in fp32 under the context's compute dtype, and a 2-byte result is the fp32 one rounded ONCE, to nearest even
 * (torch's .to(dtype)), by the epilogue that stores it.  Views of 2-byte tensors (afi_view_t.p) point at 2-byte elements, strides in elements. */
#define AFI_STORE_F32 0
#define AFI_STORE_BF16 1
#define AFI_STORE_F16 2
/* afi_generator_fwd with a 2-byte `out` (out_dtype AFI_STORE_BF16 / _F16): `x` is fp32 (widened by afi_cast_to_f32_nhwc), the workspace and
 * everything afi_generator_bwd reads are the fp32 call's, bit for bit; only the final conv's store rounds. */
int afi_generator_fwd_out16(afi_ctx_t* ctx, const afi_gen_params_t* prm, afi_view_t x, int N, int H, int W, afi_view_t out, int out_dtype,
                            float* ws, long long ws_floats, void* stream);

/* Parameters of Discriminator.Discriminators[0] (feature_patch_discriminator.py:32-41). */
typedef struct afi_disc_params {
    int F[4];               /* channels: in (256), 512, 1024, 1024 */
    float* w[3]; float* b[3];                /* Discriminators.0.n.0.{weight,bias}          n = 0..2 */
    float* gamma[3]; float* beta[3];         /* Discriminators.0.n.0.norm.{weight,bias}              */
    float* running_mean[3]; float* running_var[3];
    long long* num_batches_tracked[3];
    float* w3; float* b3;                    /* Discriminators.0.3.0.{weight [1][3][3][F3], bias[1]} */
} afi_disc_params_t;

long long afi_discriminator_fwd_ws_floats(const int F[4], int N, int H, int W);
/* ABI v7.  The same for ONE context and ONE kind of call (`training` as afi_discriminator_fwd takes it): what that call really writes.  The
 * context-free query above is an upper bound for every context and mode -- it reserves the F(4x4) input planes a training forward of blocks 1 and
 * 2 may keep for its backward's weight gradient (36 x tiles x F[n] floats each: 0.6 + 1.25 GB at 2x200x336) -- this one reserves them only
 * where the context's arithmetic, AFI_OPT_WINOGRAD_F4_FORWARD / F16_PRESPLIT and training == 1 make the forward keep them
 * (the default context: block 2 only).  Likewise the last block's activation y[2] (P x F[3] floats, the largest tensor of the network) is reserved
 * only where it is written: not under AFI_OPT_D_FUSE_TAIL (ABI v8: 0.55 GB per workspace at 2 x 200 x 336 x 1024).  Every offset that
 * afi_discriminator_ws_layout reports is the same either way (y[2] sits behind the fixed regions, the kept planes behind it), and a workspace
 * sized by either query serves afi_discriminator_fwd / _bwd under that context. */
long long afi_discriminator_fwd_ws_floats_ex(const afi_ctx_t* ctx, const int F[4], int N, int H, int W, int training);
long long afi_discriminator_bwd_ws_floats(const int F[4], int N, int H, int W);
/* Where afi_discriminator_fwd (training != 0) keeps what afi_discriminator_bwd reads, as offsets in floats into the forward
 * workspace: off12 = { c[0..2] conv outputs [P][F(n+1)], y[0..2] activations, mean[0..2], invstd[0..2] }.  For parity tooling
 * (tests feed the reference's saved activations to the backward; feature_patch_discriminator.py:35-38) and activation checkpoints. */
int afi_discriminator_ws_layout(const int F[4], int N, int H, int W, long long* off12);
/* Which activations the forward really writes, as a bit mask (bit n: y[n]).  Bits 0 and 1 are always set.  Bit 2 (y[2], which only the last
 * conv reads) is clear under AFI_OPT_D_FUSE_TAIL (the default: the mask is 3; 7 with that option off): the last conv then reads the saved conv
 * output c[2] through the block's BatchNorm affine and LeakyReLU, y = lrelu_0.2(((c - mean) * invstd) * gamma + beta) with every operation
 * rounded to fp32 on its own (the arithmetic the apply pass has; a reader of the workspace reproduces y[2] bit for bit from c[2], mean[2],
 * invstd[2] and the block's gamma / beta that way: tests/d_parity_util.py).
 * ctx may be NULL (defaults).
 * afi_discriminator_bwd must run under the same options as its forward. */
int afi_discriminator_saved_activations(const afi_ctx_t* ctx, const int F[4], int N, int H, int W);

/* logits[N,H,W] (dense) = Discriminators[0](x).  training != 0: batch statistics, running stats advance once,
 * num_batches_tracked += 1 (torch BatchNorm2d train mode);  training == 0: running statistics.
 * training == 1: afi_discriminator_bwd may follow on this workspace (the forward convs then keep the Winograd tiling whose
 * rounding does not disturb LeakyReLU mask decisions);  training == 2: train-mode statistics and logits only, no backward
 * will follow (stage-1 G phase, stage-2 generator-side terms): the convs may take the cheaper F(4x4,3x3) tiling, as in eval.
 * training == 3: as 2, but only the BatchNorm side effects are wanted (stage1_trainer.py:401-403: the G phase's D(real) call, whose
 * logits nothing reads): the running statistics and num_batches_tracked advance exactly as in mode 2; the last block's activation, the
 * last conv and the logits are not computed and `logits` may be NULL. */
int afi_discriminator_fwd(afi_ctx_t* ctx, const afi_disc_params_t* prm, afi_view_t x, int N, int H, int W, float* logits, int training,
                          float* ws, long long ws_floats, void* stream);
/* Backward (training-mode forward only).  grads: += targets (w, b, gamma, beta, w3, b3; other fields ignored).
 * dx: DENSE [N,H,W,F0] or NULL (both reference loops feed detached inputs).
 * PRECONDITION: `prm` holds the values the forward saw -- in particular gamma[n] / beta[n] must be BIT-IDENTICAL to the forward's.
 * The LeakyReLU' masks are recomputed here from the saved conv outputs c[n] (workspace) through the same affine
 * ((c - mean) * invstd) * gamma + beta, evaluated in the same order, instead of being read from the saved activations; a caller that
 * steps the BatchNorm affine between the two calls gets masks of ANOTHER affine and no error (the weights w[n] may not move either:
 * the data gradients read them).  Both reference loops run backward before any optimizer step (stage1_trainer.py:374-381,
 * stage2_trainer.py:335-342).  tests/test_gpu_d_parity.py::test_masks_recomputed_in_backward_match_the_forward counts the
 * disagreeing masks on un-nudged inputs.
 * PRECONDITION: the backward runs under the OPTIONS and the ARITHMETIC (compute dtype) its forward ran under -- on another context they must be set
 * alike.  Both passes derive from them what the workspace holds: under f16x3 the forward of blocks 1 and 2 (AFI_OPT_WINOGRAD_F4_FORWARD) keeps its
 * F(4x4) input planes, split into fp16 pieces, for the weight gradient of the same conv, and the backward reads them instead of transforming the
 * activation again; a backward that expects planes a differently-configured forward never wrote is refused where the library can see it
 * (AFI_ERR_BAD_ARG) and undefined where it cannot. */
int afi_discriminator_bwd(afi_ctx_t* ctx, const afi_disc_params_t* prm, const afi_disc_params_t* grads, afi_view_t x, int N, int H, int W,
                          const float* ws, const float* dlogits, float* dx, float* scratch, long long scratch_floats, void* stream);

/* TWO consecutive calls of the reference as one: x holds N images (N even), images [0, N/2) are the first call's batch and [N/2, N) the
 * second's -- D(real) then D(fake) in the D phase (stage1_trainer.py:349-359), D(fake) then D(real) in the G phase (:399-403).  Every
 * convolution runs once over all N images (half the launches, twice the rows per GEMM: what the small levels lack); every BatchNorm takes
 * its batch statistics over each half alone and moves the running statistics / num_batches_tracked twice, first half first, so the
 * parameters, buffers and logits come out as from the two calls (to fp32 rounding: under f16x3 the two halves share one operand scale per
 * Winograd plane -- a half whose largest magnitude lies 2^k below the other's keeps 22 - k significand bits in the FIRST conv; behind it every
 * BatchNorm has normalised the halves separately.  Pair tensors of like scale, as D(real) / D(fake) under an L1 term are).
 * Workspace sizes are those of the N-image call; `logits` / `dlogits` are [N, H, W]; the parameter gradients of both halves add up, as
 * two backward calls would leave them.  The second half's batch statistics sit behind the layout afi_discriminator_ws_layout reports. */
int afi_discriminator_fwd_paired(afi_ctx_t* ctx, const afi_disc_params_t* prm, afi_view_t x, int N, int H, int W, float* logits, int training,
                                 float* ws, long long ws_floats, void* stream);
int afi_discriminator_bwd_paired(afi_ctx_t* ctx, const afi_disc_params_t* prm, const afi_disc_params_t* grads, afi_view_t x, int N, int H, int W,
                                 const float* ws, const float* dlogits, float* dx, float* scratch, long long scratch_floats, void* stream);

/* ------------------------------------------------------------------ per-op entry points (also used by the tests) */

/* out[.., c_out] = act(alpha*conv3x3(x, w) + bias + beta*out);  w [Cout][3][3][Cin]  (generator_rdb.py:39-55,91-99,107)
 * lrelu: 0 = no activation, 1 = LeakyReLU(0.2), 2 = ReLU (used by the bench harness's guide network only) */
int afi_conv3x3_fwd(afi_ctx_t* ctx, afi_view_t x, int N, int H, int W, int Cin, const float* w, const float* bias, int Cout,
                    afi_view_t out, float alpha, float beta, int lrelu, void* stream);
/* dx = alpha*conv3x3^T(dy, w) + beta*dx, optionally times lrelu'(z) (z = the activation that produced x) */
int afi_conv3x3_dgrad(afi_ctx_t* ctx, afi_view_t dy, int N, int H, int W, int Cout, const float* w, int Cin, afi_view_t dx,
                      float alpha, float beta, afi_view_t z_or_null, void* stream);
/* dw[Cout][3][3][Cin] += alpha * sum_pix dy (x) x */
int afi_conv3x3_wgrad(afi_ctx_t* ctx, afi_view_t dy, afi_view_t x, int N, int H, int W, int Cout, int Cin, float* dw, float alpha, void* stream);
/* afi_conv3x3_fwd storing a 2-byte `out` (out_dtype AFI_STORE_BF16 / _F16).  A 2-byte output is write-only: beta != 0 is AFI_ERR_UNSUPPORTED. */
int afi_conv3x3_fwd_out16(afi_ctx_t* ctx, afi_view_t x, int N, int H, int W, int Cin, const float* w, const float* bias, int Cout,
                          afi_view_t out, int out_dtype, float alpha, float beta, int lrelu, void* stream);

/* 1x1 convs of the AFI FPN lateral merge (fpn_sr.py:79-81,152-153), w [Cout][Cin]:
 * out = act(alpha*conv1x1(x, w) + bias + beta*out + r1_scale*r1)   -- r1 = the up-sampled top-down feature (or NULL) */
int afi_conv1x1_fwd(afi_ctx_t* ctx, afi_view_t x, int N, int H, int W, int Cin, const float* w, const float* bias, int Cout, afi_view_t out,
                    float alpha, float beta, afi_view_t r1_or_null, float r1_scale, int lrelu, void* stream);
int afi_conv1x1_dgrad(afi_ctx_t* ctx, afi_view_t dy, int N, int H, int W, int Cout, const float* w, int Cin, afi_view_t dx, float alpha, float beta,
                      void* stream);
int afi_conv1x1_wgrad(afi_ctx_t* ctx, afi_view_t dy, afi_view_t x, int N, int H, int W, int Cout, int Cin, float* dw, float alpha, void* stream);
/* The data gradients with the activation's mask by kind, for a conv whose input is act(z): z_act 1 = LeakyReLU(0.2) (the factor of the
 * z_or_null forms above), 2 = ReLU (z > 0 ? 1 : 0, an exact 0 where z <= 0); z NULL = no mask.  The mask is the last factor, over the join:
 *   dx = (alpha*W^T dy + beta*dx + add_scale*add) * act'(z).
 * dx, add and z may be strided views (every second pixel).  beta != 0 reads dx only in the epilogue, by the thread that stores the element
 * (split-K forms included), so dx may be updated in place as long as it aliases neither dy nor w. */
int afi_conv1x1_dgrad_act(afi_ctx_t* ctx, afi_view_t dy, int N, int H, int W, int Cout, const float* w, int Cin, afi_view_t dx, float alpha, float beta,
                          afi_view_t add_or_null, float add_scale, afi_view_t z_or_null, int z_act, void* stream);
int afi_conv3x3_dgrad_act(afi_ctx_t* ctx, afi_view_t dy, int N, int H, int W, int Cout, const float* w, int Cin, afi_view_t dx,
                          float alpha, float beta, afi_view_t z_or_null, int z_act, void* stream);
int afi_conv3x3_wino_dgrad_act(afi_ctx_t* ctx, afi_view_t dy, int N, int H, int W, int Cout, const float* w_ohwi, int Cin, afi_view_t dx,
                               afi_view_t z_or_null, int z_act, float* ws, long long ws_floats, void* stream);
/* afi_conv1x1_dgrad storing a 2-byte `dx` (dx_dtype AFI_STORE_BF16 / _F16; beta != 0: AFI_ERR_UNSUPPORTED) -- the lateral conv's input gradient */
int afi_conv1x1_dgrad_out16(afi_ctx_t* ctx, afi_view_t dy, int N, int H, int W, int Cout, const float* w, int Cin, afi_view_t dx, int dx_dtype,
                            float alpha, float beta, void* stream);

/* The same 3x3 / stride-1 / pad-1 conv in Winograd F(2x2,3x3) form (2.25x fewer matrix-core FLOPs; large maps with many
 * channels): weight + input transforms, one batched 1x1 GEMM over the 16 transform points, output transform with the
 * epilogue.  fwd: out = conv(x, w) + bias.  dgrad: dx = conv^T(dy) * lrelu'(z) (z NULL = no mask).  ws from
 * afi_conv3x3_wino_ws_floats(N, H, W, Cin, Cout) (the same size serves both directions). */
long long afi_conv3x3_wino_ws_floats(int N, int H, int W, int Cin, int Cout);
int afi_conv3x3_wino_fwd(afi_ctx_t* ctx, afi_view_t x, int N, int H, int W, int Cin, const float* w_ohwi, const float* bias_or_null, int Cout,
                         afi_view_t out, float* ws, long long ws_floats, void* stream);
/* afi_conv3x3_wino_fwd storing a 2-byte `out` (out_dtype AFI_STORE_BF16 / _F16), rounded in the output transform */
int afi_conv3x3_wino_fwd_out16(afi_ctx_t* ctx, afi_view_t x, int N, int H, int W, int Cin, const float* w_ohwi, const float* bias_or_null, int Cout,
                               afi_view_t out, int out_dtype, float* ws, long long ws_floats, void* stream);
/* inference form: out = act(conv + bias), act 0 none / 1 LeakyReLU(0.2) / 2 ReLU; no backward will follow, so maps of >= 8192 pixels
 * take the F(4x4,3x3) tiling (4x fewer multiplies; max-norm rounding 3e-6 .. 6e-6 of the output scale at 128 .. 256 channels against F(2x2)'s
 * 5e-7 .. 8e-7, what a plain fp32 evaluation of the same transforms loses: tests/test_gpu_wino.py) */
int afi_conv3x3_wino_infer(afi_ctx_t* ctx, afi_view_t x, int N, int H, int W, int Cin, const float* w_ohwi, const float* bias_or_null, int Cout,
                           afi_view_t out, int act, float* ws, long long ws_floats, void* stream);
int afi_conv3x3_wino_dgrad(afi_ctx_t* ctx, afi_view_t dy, int N, int H, int W, int Cout, const float* w_ohwi, int Cin, afi_view_t dx,
                           afi_view_t z_or_null, float* ws, long long ws_floats, void* stream);

/* weight gradient of the same conv in Winograd F(3x3,2x2) form (shares the input transform with the forward):
 * dw[Cout][3][3][Cin] += alpha * sum_pix dy (x) x */
int afi_conv3x3_wino_wgrad(afi_ctx_t* ctx, afi_view_t dy, afi_view_t x, int N, int H, int W, int Cout, int Cin, float* dw, float alpha, float* ws,
                           long long ws_floats, void* stream);

/* Conv2d(k=3, stride=2, padding=1) on [N,Hi,Wi,Cin] -> [N,Ho,Wo,Cout], Ho = ceil(Hi/2): the PAFPN bottom-up downsample conv
 * with its fused merge (pafpn_sr.py:105-117,177-183):
 *   a = act(conv(x,w) + bias)            -> act_out (or NULL; kept for the ReLU backward)
 *   out = post_scale*a + r_scale*r       (r NULL = no residual)
 * dgrad: dx[N,Hi,Wi,Cin] = alpha*conv^T(dy) + beta*dx, run as four parity-phase GEMMs (9 taps in total).
 * wgrad: dw[Cout][3][3][Cin] += alpha * sum_pix dy (x) x. */
int afi_conv3x3s2_fwd(afi_ctx_t* ctx, afi_view_t x, int N, int Hi, int Wi, int Cin, const float* w_ohwi, const float* bias_or_null, int Cout,
                      afi_view_t out, int act, afi_view_t act_out_or_null, float post_scale, afi_view_t r_or_null, float r_scale,
                      void* stream);
int afi_conv3x3s2_dgrad(afi_ctx_t* ctx, afi_view_t dy /*[N,Ho,Wo,Cout]*/, int N, int Hi, int Wi, int Cout, const float* w_ohwi, int Cin,
                        afi_view_t dx, float alpha, float beta, void* stream);
int afi_conv3x3s2_wgrad(afi_ctx_t* ctx, afi_view_t dy, afi_view_t x /*[N,Hi,Wi,Cin]*/, int N, int Hi, int Wi, int Cout, int Cin, float* dw,
                        float alpha, void* stream);
/* out[i] = scale * g[i] * (act[i] > 0): gradient through the ReLU of pafpn_sr.py:178 from its kept output (n % 4 == 0) */
int afi_relu_bwd(const float* g, const float* act, float* out, long long n, float scale, void* stream);

/* BiFPN_AFIGAN inference pieces around the interpolator (bifpn_sr.py:531-733, bifpn_layers/wrappers.py:172-252, activations.py):
 *   afi_dwconv3x3_fwd        SeparableConv2d.depthwise: 3x3, stride 1, zero pad 1, no bias; w9c = [9][C] (tap-major)
 *   afi_maxpool3s2_same_fwd  MaxPool2d(3, 2, "static_same"): zero pad right/bottom by 1 (the zeros take part in the max),
 *                            out dense [N, (H-2)/2+1, (W-2)/2+1, C]
 *   afi_fuse_swish_fwd       out = swish(w[0]*a + w[1]*b (+ w[2]*c)); a, b, c, out dense and equal-sized, w a DEVICE pointer
 * The depthwise conv and both max-pool forwards read x, w9c and write out with 16-byte accesses: C % 4 == 0, x.p / w9c / out 16-byte
 * aligned and the view's strides multiples of 4 (AFI_ERR_UNSUPPORTED otherwise, as afi_nearest_nhwc).
 * The pointwise 1x1 conv (+ folded eval-mode norm) is afi_conv1x1_fwd. */
int afi_dwconv3x3_fwd(afi_view_t x, int N, int H, int W, int C, const float* w9c, float* out, void* stream);
int afi_maxpool3s2_same_fwd(afi_view_t x, int N, int H, int W, int C, float* out, void* stream);
int afi_fuse_swish_fwd(const float* a, const float* b, const float* c_or_null, const float* w_dev, float* out, long long n,
                       void* stream);

/* BiFPN_AFIGAN under autograd (the same node, training mode): the backward of the three pieces above.  No atomics: every reduction is
 * two-stage in a fixed order.  The depthwise INPUT gradient is afi_dwconv3x3_fwd on dy with the taps reversed (w9c rows 8..0); the
 * pointwise conv is afi_conv1x1_{dgrad,wgrad}; the train-mode norm is afi_bn_stats_ex + afi_bn_apply_fwd + afi_bn_bwd.
 *   afi_fuse_swish_bwd           ds = dout * swish'(w.{a,b,c});  d{a,b,c} = w_k * ds (each optional), dw[2 or 3] = sum ds * {a,b,c}
 *                                (MemoryEfficientSwish.backward, bifpn_layers/activations.py); scratch: afi_fuse_swish_bwd_scratch_floats()
 *   afi_dwconv3x3_wgrad          dw9c[t][c] = sum_pixels dy[p][c] * x[p + tap t][c]; dy, x dense [N,H,W,C];
 *                                scratch: afi_dwconv3x3_wgrad_scratch_floats(C)
 *   afi_maxpool3s2_same_fwd_idx  the forward, also keeping idx[N,Ho,Wo,C] (one byte per element, 4-byte aligned): tap 3*dy+dx of the
 *                                first maximum in scan order, which is where torch's max_pool2d sends the gradient
 *   afi_maxpool3s2_same_bwd      dx dense [N,H,W,C] = gather of dout over the windows whose argmax is the element (a window won by the
 *                                zero pad sends its gradient nowhere, as F.pad's backward drops it) */
long long afi_fuse_swish_bwd_scratch_floats(void);
int afi_fuse_swish_bwd(const float* a, const float* b, const float* c_or_null, const float* w_dev, const float* dout, float* da_or_null,
                       float* db_or_null, float* dc_or_null, float* dw_or_null, long long n, float* scratch, void* stream);
long long afi_dwconv3x3_wgrad_scratch_floats(int C);
int afi_dwconv3x3_wgrad(const float* dy, const float* x, int N, int H, int W, int C, float* dw9c, float* scratch, void* stream);
int afi_maxpool3s2_same_fwd_idx(afi_view_t x, int N, int H, int W, int C, float* out, unsigned char* idx, void* stream);
int afi_maxpool3s2_same_bwd(const float* dout, const unsigned char* idx, int N, int H, int W, int C, float* dx, void* stream);

/* ConvTranspose2d(k=6,s=2,p=2) (generator_rdb.py:101-105) on the packed weight wp[4*Cout][3][3][Cin] */
int afi_convT6s2_pack_weight(const float* w_iohw, float* wp, int Cin, int Cout, void* stream);
int afi_convT6s2_unpack_wgrad(const float* dwp, float* dw_iohw, int Cin, int Cout, void* stream);   /* dw += */
int afi_convT6s2_fwd(afi_ctx_t* ctx, afi_view_t x, int N, int H, int W, int Cin, const float* wp, const float* bias, int Cout,
                     afi_view_t out /*[N,2H,2W,Cout]*/, int lrelu, void* stream);
int afi_convT6s2_dgrad(afi_ctx_t* ctx, afi_view_t dy /*[N,2H,2W,Cout]*/, int N, int H, int W, int Cout, const float* wp, int Cin,
                       afi_view_t dx, afi_view_t z_or_null, void* stream);
int afi_convT6s2_wgrad(afi_ctx_t* ctx, afi_view_t dy, afi_view_t x, int N, int H, int W, int Cout, int Cin, float* dwp, float alpha, void* stream);

/* out (dense [N,2H,2W,C]) = beta*out + bilinear_x2(x), align_corners=False (generator_rdb.py:125) */
int afi_bilinear2x_add_fwd(afi_view_t x, int N, int H, int W, int C, float beta, float* out, void* stream);
int afi_bilinear2x_add_bwd(const float* dout, int N, int H, int W, int C, float beta, float* dx, void* stream);

/* train-mode BatchNorm2d over a dense [P][C] matrix + LeakyReLU(0.2)  (feature_patch_discriminator.py:35-38) */
long long afi_reduce_scratch_floats(int C);
int afi_bn_stats(const float* x, long long P, int C, float* mean, float* invstd, float* var_biased_or_null,
                 float* running_mean_or_null, float* running_var_or_null, float* scratch, void* stream);
int afi_bn_apply_lrelu_fwd(const float* x, float* y, const float* mean, const float* invstd, const float* gamma,
                           const float* beta, long long P, int C, void* stream);
/* The same two passes for a norm with its own eps / momentum and no activation behind it (BiFPN: eps 1e-3, momentum 0.01,
 * bifpn_sr.py:279-280): statistics (+ running-stat update and num_batches_tracked += 1 when given), then
 * y = lrelu_slope((x - mean) * invstd * gamma + beta) with slope 1 = the plain affine.  Backward: afi_bn_bwd. */
int afi_bn_stats_ex(const float* x, long long P, int C, float eps, float momentum, float* mean, float* invstd, float* var_biased_or_null,
                    float* running_mean_or_null, float* running_var_or_null, long long* num_batches_tracked_or_null, float* scratch,
                    void* stream);
int afi_bn_apply_fwd(const float* x, float* y, const float* mean, const float* invstd, const float* gamma, const float* beta,
                     long long P, int C, float slope, void* stream);
int afi_bn_bwd(const float* g, const float* x, float* dx, const float* mean, const float* invstd, const float* gamma,
               float* dgamma, float* dbeta, long long P, int C, float* scratch, void* stream);
/* afi_bn_bwd in two halves, for a norm whose batch statistics span several ranks (norm = "SyncBN", bifpn_sr.py:210,279-280; torch.nn.SyncBatchNorm):
 * the sums of this rank's rows -- sums2C[0..C) = sum g, sums2C[C..2C) = sum g * xhat, xhat from the GLOBAL mean / invstd; dbeta / dgamma (optional) +=
 * them, per rank as torch keeps them --, which the caller all-reduces, then dx = gamma invstd (g - sums[0] / P_total - xhat sums[1] / P_total) over
 * this rank's P rows.  scratch: afi_reduce_scratch_floats(C). */
int afi_bn_bwd_sums(const float* g, const float* x, const float* mean, const float* invstd, float* dgamma_or_null, float* dbeta_or_null, float* sums2C,
                    long long P, int C, float* scratch, void* stream);
int afi_bn_bwd_apply(const float* g, const float* x, float* dx, const float* mean, const float* invstd, const float* gamma, const float* sums2C,
                     long long P, long long P_total, int C, void* stream);
/* db[C] += alpha * column sums of the [P][C] matrix g with row stride ld */
int afi_colsum_accum(const float* g, long long P, int C, long long ld, float alpha, float* db, float* scratch, void* stream);

/* nn.BCEWithLogitsLoss() mean vs a constant target (stage1_trainer.py:358-359,408):  *loss += lscale*bce;
 * dz (or NULL) = gscale * d bce / dz */
int afi_bce_logits_fwd_bwd(const float* z, long long n, float target, float lscale, float* loss, float gscale, float* dz, void* stream);
/* F.l1_loss mean over the common crop [N,h,w,C] of a and b (stage1_trainer.py:410,437-443): *loss += lscale*l1;
 * da (or NULL): DENSE [N,Ha,Wa,C] gradient w.r.t. a (zeros outside the crop) */
int afi_l1_fwd_bwd(afi_view_t a, afi_view_t b, int N, int h, int w, int C, int Ha, int Wa, float lscale, float* loss,
                   float gscale, float* da, void* stream);

/* multi-tensor SGD with momentum (torch.optim.SGD as built by detectron2 build_optimizer, stage1_trainer.py:110-114):
 *   d = g*gscale + wd*p ; buf = momentum*buf + d ; p -= lr*buf.    descs: DEVICE array of afi_sgd_desc_t */
typedef struct afi_sgd_desc { float* p; const float* g; float* m; long long n; float wd; float pad_; } afi_sgd_desc_t;
int afi_sgd_momentum_step(const afi_sgd_desc_t* descs_dev, int ntensors, long long max_n, float lr, float momentum,
                          float gscale, void* stream);
int afi_scale_inplace(float* p, long long n, float s, void* stream);

/* Weight gradients of convs that ran on weights folded with their FrozenBN (w' = w * s[o], s = gamma / sqrt(var + eps)), back to the
 * parameter: grad[o][i][kh][kw] = fmaf(s[o], dw'[o][kh][kw][i], grad[o][i][kh][kw]) -- dw' in the kernels' [O][k][k][I] memory ([O][I] for
 * k = 1), grad in the parameter's [O][I][k][k].  One launch over a DEVICE array of descriptors (all trainable convs of a network); every
 * element has one owner: no atomics, bit-identical between runs.  max_oi: the largest O * ceil(I / 32) of the descriptors. */
typedef struct afi_unfold_desc { const float* dw; float* grad; const float* s; int O; int I; int k; int pad_; } afi_unfold_desc_t;
int afi_frozen_wgrad_unfold(const afi_unfold_desc_t* descs_dev, int ntensors, long long max_oi, void* stream);

/* The detector's optimiser step (afigan_amd/detector_optim.py): torch.optim.SGD as detectron2 v0.1.1's build_optimizer configures it, for every
 * trainable tensor in one launch, with the FrozenBN refold of the trainable frozen.Conv2d weights in the same pass.  Per element, in fp32:
 *   d = fmaf(wd, p, g * gscale);  m = fmaf(momentum, m, d);  p = fmaf(-lr, m, p)          lr and wd per tensor
 * p, g, m: n dense floats in one memory order (the parameter's own); 16-byte accesses where the three pointers allow, scalar otherwise.
 * A fold entry (fold_out != NULL; a contiguous [O][I][k][k] weight, k 1 or 3, n = O I k k) also gets
 *   fold_out = (float)((double)p_new * s64[o])      s64: DEVICE fp64 [O], gamma / sqrt(var + eps) of the conv's FrozenBN
 * written as [O][I] for k = 1 and as the kernels' [O][kh][kw][I] for k = 3: one fp64 product rounded once, frozen.fold_conv's expression.
 * The table is given twice: descs_host is checked (AFI_ERR_BAD_ARG: a null table, ntensors <= 0 or > 65535, a live entry without p, g or m, a
 * fold entry without s64, with k other than 1 or 3, or with n != O I k k), descs_dev is what the kernel reads.  n == 0 entries are skipped.
 * Work is cut into units, afi_detector_sgd_units per tensor (4096 elements; 4 pieces of one output channel x 32 input channels of a k = 3 fold
 * entry).  unit_off_dev == NULL: a (min(512, max_units), ntensors) grid, max_units the largest unit count of the table.  Otherwise a flat grid
 * of min(2048, total_units) blocks over all units, unit_off_dev a DEVICE int [ntensors + 1] = the exclusive prefix of the unit counts and
 * total_units its last element.  One owner per element, no atomics: results are bit-identical between runs and between the two grids. */
typedef struct afi_det_sgd_desc {
    float* p; const float* g; float* m; long long n; float lr; float wd;
    float* fold_out; const double* s64; int O; int I; int k; int pad_;
} afi_det_sgd_desc_t;
long long afi_detector_sgd_units(long long n, int O, int I, int k, int fold);
int afi_detector_sgd_step(const afi_det_sgd_desc_t* descs_host, const afi_det_sgd_desc_t* descs_dev, int ntensors, long long max_units,
                          const int* unit_off_dev, long long total_units, float momentum, float gscale, void* stream);

/* layout changes at the detectron2 boundary: [N][C][P] <-> [N][P][C] */
int afi_nchw_to_nhwc(const float* in, float* out, int N, int C, int P, void* stream);
int afi_nhwc_to_nchw(const float* in, float* out, int N, int C, int P, void* stream);
/* storage-dtype casts at the module boundary.  to_f32: dst = the DENSE fp32 [N][H][W][C] copy of src (src_dtype AFI_STORE_*), whose element
 * (n, c, y, x) is at src + n*sN + c*sC + y*sH + x*sW (strides in elements; exact).  from_f32: dst = the DENSE 2-byte [N][H][W][C] copy of the
 * pixel-major fp32 view src (dst_dtype AFI_STORE_BF16 / _F16), rounded to nearest even.  Buffers need only their element's alignment:
 * 8- / 16-byte vector accesses are used where src, dst, C and the strides allow them, one element per thread otherwise. */
int afi_cast_to_f32_nhwc(const void* src, int src_dtype, int N, int C, int H, int W, long long sN, long long sC, long long sH, long long sW,
                         float* dst, void* stream);
int afi_cast_from_f32_nhwc(afi_view_t src, int N, int H, int W, int C, void* dst, int dst_dtype, void* stream);

/* ------------------------------------------------------------------ dual-scale data path
 * afi_resize_bilinear_u8: what ResizeTransform.apply_image does to a uint8 image under the reference's DatasetMapper
 * (afigan/engine/dataset_mapper.py:85-107; target sizes from afigan/engine/transform_gen.py:198-217 for `image` and
 * :542-543 for `image_x0.5`): Pillow's antialiased BILINEAR resample, bit-exact (22-bit fixed-point coefficients, horizontal
 * pass rounded to uint8, then vertical pass), followed by the shared HFlipTransform when `hflip` != 0.
 *   src [H0][W0][C] uint8 (C = 1 or 3: Pillow modes L / RGB), dst [H1][W1][C] (out_chw == 0) or [C][H1][W1] (out_chw != 0, the mapper's tensor layout),
 *   ws  >= afi_resize_bilinear_u8_ws_bytes(...) bytes of device scratch (the coefficient tables).
 * afi_normalize_pad_u8: RCNN_FPN_only.forward's per-image normaliser and ImageList.from_tensors padding
 * (afigan/modeling/meta_arch/rcnn_only.py:36-39): out[c][y][x] = (img[c][y][x] - mean[c]) / std[c] in fp32 for y < H, x < W and
 * 0 up to Hp x Wp; img is [C][H][W] uint8 on the device, mean/std are HOST arrays of C floats, out is one [C][Hp][Wp] slot of the batch. */
/* afi_dual_scale_u8: both images of one sample in two launches -- `image` [H1,W1] and `image_x0.5` [H2,W2], each resized from
 * the same ORIGINAL src (dataset_mapper.py:103-105) with its own flip flag (equal when the flip is shared, transform_gen.py:546-554). */
long long afi_resize_bilinear_u8_ws_bytes(int H0, int W0, int C, int H1, int W1);
int afi_resize_bilinear_u8(const unsigned char* src, int H0, int W0, int C, unsigned char* dst, int H1, int W1, int hflip,
                           int out_chw, void* ws, long long ws_bytes, void* stream);
long long afi_dual_scale_u8_ws_bytes(int H0, int W0, int C, int H1, int W1, int H2, int W2);
int afi_dual_scale_u8(const unsigned char* src, int H0, int W0, int C, unsigned char* image, int H1, int W1, int hflip,
                      unsigned char* image_r, int H2, int W2, int hflip_r, int out_chw, void* ws, long long ws_bytes, void* stream);
int afi_normalize_pad_u8(const unsigned char* img_chw, int C, int H, int W, const float* mean, const float* std_,
                         float* out, int Hp, int Wp, void* stream);

/* ------------------------------------------------------------------ frozen ResNet-FPN guide (afigan_amd/resnet_guide.py)
 * The guide network of stages 1 and 2 (RCNN_FPN_only over detectron2's build_resnet_fpn_backbone), forward only.  Its 1x1 convs are
 * afi_conv1x1_fwd, its 3x3 convs afi_conv3x3_fwd / afi_conv3x3_wino_infer / afi_conv3x3s2_fwd; these two cover the rest.
 * afi_resnet_stem_fwd: BasicStem in one kernel -- out = max_pool2d(relu(conv2d(x, w, bias, stride 2, pad 3)), 3, stride 2, pad 1), torch's
 *   padding (zeros for the conv, -inf for the pool).  x dense NCHW [N][3][H][W] fp32 (the normalised, padded batch); w dense [64][3][7][7]
 *   and bias[64] with the FrozenBN affine folded in; out dense [N][Ho][Wo][64], Ho = ceil(ceil(H/2)/2).  fp32 FMA chains; the conv map
 *   is never written.
 * afi_nearest_nhwc: out dense [N][Ho][Wo][C] = x[n][oy*down/up][ox*down/up][c], Ho = ceil(H*up/down): F.interpolate(scale_factor=2,
 *   mode="nearest") with up = 2, down = 1 (the FPN top-down addend), max_pool2d(1, stride 2) with up = 1, down = 2 (LastLevelMaxPool).
 *   C % 4 == 0, x and out 16-byte aligned, view strides multiples of 4 (AFI_ERR_UNSUPPORTED otherwise). */
int afi_resnet_stem_fwd(const float* x, int N, int H, int W, const float* w, const float* bias, float* out, void* stream);
int afi_nearest_nhwc(afi_view_t x, int N, int H, int W, int C, int up, int down, float* out, void* stream);

/* ------------------------------------------------------------------ forward 1x1 conv of FROZEN weights on the bf16 matrix cores (csrc/frozen1x1.hip)
 * out = act(alpha*conv1x1(x, w) + bias + add_scale*add), act 0 / 1 / 2 as afi_conv1x1_fwd, in the bf16x6 arithmetic (every fp32 operand split
 * exactly into three bf16, six products summed smallest first into fp32): for the large maps of a frozen guide, whose weights are turned into
 * a pre-split image ONCE.  fp32 in memory on both sides; no atomics, no scratch: bit-reproducible and capturable into a graph.
 * afi_frozen1x1_image_bytes: size of the image of w [Cout][Cin] (0 unless both are positive multiples of 32).
 * afi_conv1x1_frozen_image: one launch that writes it (image 16-byte aligned, image_bytes >= the size above: AFI_ERR_WORKSPACE otherwise).
 * afi_frozen1x1_plan (host only, no device): AFI_OK when afi_conv1x1_frozen_fwd takes the problem, and then plan[0..12) = M, BM, BN, KC (the
 *   64 x BN output tile and the channels per K chunk), row tiles, column tiles, grid, LDS bytes, byte extents of x / out / image, x dense;
 *   AFI_ERR_UNSUPPORTED (nothing would be launched; the caller runs afi_conv1x1_fwd) unless: Cin % 32 == 0 and Cout % 32 == 0; x is every
 *   s-th pixel (s >= 1, both directions) of a pixel-major tensor of Cin channels (x.sW = s Cin, x.sH >= s ((W-1) s + 1) Cin) -- a channel
 *   slice of a wider tensor is refused --; out dense [N][H][W][Cout] and add, if given, dense like out; every byte extent below 2 GB.
 * afi_conv1x1_frozen_fwd: any M = N H W >= 1 that the plan accepts; `image` must hold the image of this conv's w.  ctx is unused (reserved). */
long long afi_frozen1x1_image_bytes(int Cout, int Cin);
int afi_frozen1x1_plan(int N, int H, int W, int Cin, int Cout, long long x_sN, long long x_sH, long long x_sW, long long o_sN, long long o_sH,
                       long long o_sW, int has_add, long long a_sN, long long a_sH, long long a_sW, long long* plan);
int afi_conv1x1_frozen_image(afi_ctx_t* ctx, const float* w, int Cout, int Cin, void* image, long long image_bytes, void* stream);
int afi_conv1x1_frozen_fwd(afi_ctx_t* ctx, afi_view_t x, int N, int H, int W, int Cin, const void* image, const float* bias, int Cout, afi_view_t out,
                           float alpha, afi_view_t add_or_null, float add_scale, int act, void* stream);

/* ------------------------------------------------------------------ frozen ResNeSt bottom-up (afigan_amd/resnest_backbone.py)
 * detectron2-ResNeSt (radix 2, cardinality 1, deep stem, AVD, avg_down), forward only.  Its 1x1 convs are afi_conv1x1_fwd, its stride-1 3x3
 * convs afi_conv3x3_fwd / afi_conv3x3_wino_infer (a split-attention conv: one launch per radix group, through channel views); these cover
 * the rest.  All outputs are dense pixel-major; channel counts are multiples of 4, views 16-byte aligned with strides multiples of 4
 * (AFI_ERR_UNSUPPORTED otherwise).  No atomics: every sum has a fixed order.
 * afi_resnest_stem_fwd: the deep stem's first conv, out [N][Ho][Wo][Cout] = relu(conv2d(x, w, bias, stride 2, pad 1)), Ho = ceil(H/2);
 *   x dense NCHW [N][3][H][W] fp32, w dense [Cout][3][3][3] in (O, kh, kw, I) order with the norm folded in, Cout <= 128.
 * afi_resnest_pool_nhwc: out [N][Ho][Wo][C] of x [N][H][W][C] by `mode`:
 *   AFI_POOL_MAX3S2P1     max_pool2d(3, 2, 1), -inf padding; Ho = ceil(H/2)                                        (the stem)
 *   AFI_POOL_AVG3S2P1     AvgPool2d(3, 2, padding 1), count_include_pad: always / 9; Ho = ceil(H/2)                 (AVD)
 *   AFI_POOL_AVG2S2_CEIL  AvgPool2d(2, 2, ceil_mode, count_include_pad=False): / the pixels covered; Ho = ceil(H/2) (avg_down)
 * Split attention over the two radix splits s0, s1 ([N][H][W][C] each, C = the group width, after bn0 + ReLU) in three passes:
 *   afi_resnest_splat_gap      part = per-chunk channel sums of s0 + s1, [N][chunks][C]; part_floats >= afi_resnest_splat_ws_floats.
 *   afi_resnest_splat_attn     att [N][2C]: gap = (sum of the chunks, in order) / (H*W); h = relu(w1 gap + b1) (w1 [I][C], bn1 folded);
 *                              z = w2 h + b2 (w2 [2C][I]); (att[c], att[C+c]) = softmax(z[c], z[C+c]).  C <= 1024, I % 4 == 0.
 *   afi_resnest_splat_combine  out = att[c] s0 + att[C+c] s1 ([N][H][W][C], avd 0), or its AvgPool2d(3, 2, padding 1) ([N][ceil(H/2)][ceil(W/2)][C],
 *                              avd 1: the AVD layer of a stride-2 block, fused). */
#define AFI_POOL_MAX3S2P1 0
#define AFI_POOL_AVG3S2P1 1
#define AFI_POOL_AVG2S2_CEIL 2
int afi_resnest_stem_fwd(const float* x, int N, int H, int W, const float* w, const float* bias, int Cout, float* out, void* stream);
int afi_resnest_pool_nhwc(afi_view_t x, int N, int H, int W, int C, int mode, float* out, void* stream);
long long afi_resnest_splat_ws_floats(int N, int H, int W, int C);
int afi_resnest_splat_gap(afi_view_t s0, afi_view_t s1, int N, int H, int W, int C, float* part, long long part_floats, void* stream);
int afi_resnest_splat_attn(const float* part, int N, int H, int W, int C, int I, const float* w1, const float* b1, const float* w2,
                           const float* b2, float* att, void* stream);
int afi_resnest_splat_combine(afi_view_t s0, afi_view_t s1, int N, int H, int W, int C, const float* att, int avd, float* out, void* stream);

/* ------------------------------------------------------------------ the ResNeSt bottom-up in training
 * The backward of split attention and of the two average pools; a block's convs go back through the conv entry points above.  With
 * g = mean_HW(s0 + s1) [N][C], h = relu(w1 g + b1) [N][I] (bn1 folded), z = w2 h + b2, (a0, a1) = the pair softmax (att), u = a0 s0 + a1 s1 and
 * out = avd ? AvgPool2d(3, 2, 1)(u) : u, dout [N][Ho][Wo][C] is out's cotangent (Ho = avd ? ceil(H/2) : H) and du, u's, is dout itself or, with
 * avd, the transposed pool GATHERED: a u pixel adds the 1, 2 or 4 dout pixels whose windows hold it (ascending) and divides by 9; du is never
 * stored.  C % 4 == 0, C <= 1024, I % 4 == 0, I <= 2048, N <= 65535, every pointer and view 16-byte aligned with strides multiples of 4
 * (AFI_ERR_UNSUPPORTED otherwise).  No atomics: every sum has one fixed order, every result is bit-identical from run to run.
 *   afi_resnest_splat_attn_keep    afi_resnest_splat_attn (same kernel, bit-identical att) also storing g and h.
 *   afi_resnest_splat_bwd_dots     part [N][chunks][2][C] = per-chunk sums over pixels of du s0 and du s1, on afi_resnest_splat_gap's chunks,
 *                                  accumulated in fp64 and rounded once (da0 - da1 cancels in the next pass);
 *                                  part_floats >= afi_resnest_splat_bwd_ws_floats (AFI_ERR_WORKSPACE otherwise).
 *   afi_resnest_splat_bwd_attn     one block per image: da_r = the chunks of `part` in order; dz [N][2C]: dz0 = a0 a1 (da0 - da1), dz1 = -dz0;
 *                                  dh [N][I] = (w2^T dz) [h > 0]; dg [N][C] = w1^T dh / (H W).
 *   afi_resnest_splat_bwd_params   dw2 [2C][I] += sum_n dz_n (x) h_n, db2 [2C] += sum_n dz_n, dw1 [I][C] += s1 * sum_n dh_n (x) g_n,
 *                                  db1 [I] += s1 * sum_n dh_n: the gradients of the PARAMETERS (s1 [I] is bn1's fold scale), n ascending.
 *   afi_resnest_splat_bwd_combine  ds_r = (a_r du + dg) [s_r > 0] for r = 0, 1, written through the views ds0, ds1 (exact zeros where masked).
 *   afi_resnest_pool_bwd           dx = (beta dx + pool^T(dy)) [* (z > 0)] for x [N][H][W][C] (dx, z views; dy dense [N][ceil(H/2)][ceil(W/2)][C]):
 *                                  AFI_POOL_AVG2S2_CEIL dy / the pixels its window covered; AFI_POOL_AVG3S2P1 the gather above; dx is read only
 *                                  with beta != 0.  AFI_POOL_MAX3S2P1: AFI_ERR_UNSUPPORTED (the max-pool's backward does not exist). */
int afi_resnest_splat_attn_keep(const float* part, int N, int H, int W, int C, int I, const float* w1, const float* b1, const float* w2,
                                const float* b2, float* att, float* g, float* h, void* stream);
long long afi_resnest_splat_bwd_ws_floats(int N, int H, int W, int C);
int afi_resnest_splat_bwd_dots(afi_view_t dout, afi_view_t s0, afi_view_t s1, int N, int H, int W, int C, int avd, float* part,
                               long long part_floats, void* stream);
int afi_resnest_splat_bwd_attn(const float* part, int N, int H, int W, int C, int I, const float* att, const float* h, const float* w1,
                               const float* w2, float* dz, float* dh, float* dg, void* stream);
int afi_resnest_splat_bwd_params(const float* dz, const float* dh, const float* g, const float* h, const float* s1, int N, int C, int I,
                                 float* dw1, float* db1, float* dw2, float* db2, void* stream);
int afi_resnest_splat_bwd_combine(afi_view_t dout, afi_view_t s0, afi_view_t s1, int N, int H, int W, int C, const float* att, const float* dg,
                                  int avd, afi_view_t ds0, afi_view_t ds1, void* stream);
int afi_resnest_pool_bwd(const float* dy, int N, int H, int W, int C, int mode, afi_view_t dx, float beta, afi_view_t z_or_null, void* stream);

/* ------------------------------------------------------------------ frozen Swin Transformer bottom-up (afigan_amd/swin_backbone.py)
 * SwinTransformer (patch 4, head dim 32, window 7 or 12, no APE), forward only.  Its linears are afi_conv1x1_fwd over pixel-major tokens;
 * these cover the rest.  Outputs are dense pixel-major, channel counts multiples of 4, views 16-byte aligned with strides multiples of 4
 * (AFI_ERR_UNSUPPORTED otherwise).  No atomics.
 * afi_swin_patch_embed: out [N][ceil(H/4)][ceil(W/4)][C] = LayerNorm(conv2d(pad(x), w, bias, stride 4)) with (gamma, beta, eps); x dense NCHW
 *   [N][3][H][W] fp32 zero-padded on the right / bottom to multiples of 4, w dense [C][3][4][4]; C <= 256.
 * afi_swin_layernorm: merge 0: out [N][H][W][C] = LayerNorm over the channels of x [N][H][W][C] (biased variance, eps), gamma / beta [C].
 *   merge 1 (PatchMerging): out [N][ceil(H/2)][ceil(W/2)][4C] = LayerNorm(cat(x[0::2,0::2], x[1::2,0::2], x[0::2,1::2], x[1::2,1::2])) of x
 *   zero-padded to even H, W; gamma / beta [4C].  The normalised width (C or 4C) is at most 3072.
 * afi_swin_gelu: x[i] = x[i] / 2 (1 + erf(x[i] / sqrt 2)) in place, n % 4 == 0.
 * afi_swin_window_attn: out dense [N][H][W][C] of qkv [N][H][W][3C] (channel s C + 32 head + d, s = q, k, v): window multi-head attention
 *   of window `window` (7 or 12) over the map zero-padded to multiples of it, rolled by -shift (0 <= shift < window), padded tokens' q / k /
 *   v = qkv_bias [3C]; softmax(q k^T / sqrt 32 + bias_img[head] + mask) v, bias_img dense [C/32][NP][NP] (NP = ceil(window^2 / 16) 16;
 *   entries past window^2 unused), mask -100 between tokens of different shift regions when shift > 0; written un-rolled and cropped. */
int afi_swin_patch_embed(const float* x, int N, int H, int W, const float* w, const float* bias, const float* gamma, const float* beta, float eps,
                         int C, float* out, void* stream);
int afi_swin_layernorm(afi_view_t x, int N, int H, int W, int C, const float* gamma, const float* beta, float eps, int merge, float* out,
                       void* stream);
int afi_swin_gelu(float* x, long long n, void* stream);
int afi_swin_window_attn(afi_view_t qkv, int N, int H, int W, int C, const float* qkv_bias, const float* bias_img, int window, int shift,
                         float* out, void* stream);

/* ------------------------------------------------------------------ training the Swin bottom-up (afigan_amd/swin_backbone.py)
 * The backward of the entry points above; the linears' gradients are afi_conv1x1_dgrad / _wgrad / afi_colsum_accum.  fp32, the constraints of
 * the forward (AFI_ERR_UNSUPPORTED otherwise), no atomics: every result is bit-identical from run to run.
 * afi_swin_layernorm_bwd: the backward of afi_swin_layernorm(x, ..., merge) for dy dense [N][Ho][Wo][Ct] (Ct = C, or 4C with merge): x-hat and
 *   rstd are recomputed from x;  dx = beta dx + rstd (g - mean(g) - x-hat mean(g x-hat)), g = dy gamma, a view [N][H][W][C] (with merge the
 *   four source pixels of every output token; quadrants past an odd edge are dropped); dx.p NULL: no dx.  dgamma / dbeta [Ct] (both or
 *   neither) += sum over tokens of dy x-hat / dy: per-wave partials in ws (afi_swin_layernorm_bwd_ws_floats floats, 16-byte aligned; less:
 *   AFI_ERR_WORKSPACE; read only after being written), added in fp64 in one fixed order (16 slices of consecutive rows, each ascending, then
 *   the slice sums ascending).  afi_swin_layernorm_bwd_vecs(Ct): the float4s per
 *   lane (2, 6 or 12) of the kernel instantiation a token of Ct channels runs on, -1 for a Ct the kernel does not take.
 * afi_swin_gelu_bwd: dx[i] = dy[i] (Phi(x[i]) + x[i] phi(x[i])), x the GELU's input; dx may be dy; n % 4 == 0.
 * afi_swin_window_attn_bwd: for afi_swin_window_attn(qkv, ...) and dout, a view [N][H][W][C]: dqkv dense [N][Hp][Wp][3C] over the PADDED map
 *   (Hp, Wp = H, W rounded up to the window; Hp Wp 3C < 2^31), every position written: a padded position's entries are gradients of qkv_bias, so
 *   d qkv_bias is the column sum of all of dqkv and the [H][W] crop is the gradient of qkv.  ds_part [N][groups][C/32][NP][NP] (groups =
 *   afi_swin_window_attn_bwd_groups, floats = afi_swin_window_attn_bwd_ws_floats; fewer: AFI_ERR_WORKSPACE): the sum of dS = P (dP - rowsum(dP P))
 *   over the windows of a group (at most 8 consecutive windows), every entry written.
 * afi_swin_bias_table_bwd: dtable [R][heads] += sum over the nparts = N groups partials and the pairs (i, j) of table row r of ds_part[.][h][i][j],
 *   in fp64 in a fixed order: first the partials of every (h, i, j) in ascending order (images, then groups of windows) into ws, heads NP NP
 *   doubles (afi_swin_bias_table_bwd_ws_floats floats, 16-byte aligned; fewer: AFI_ERR_WORKSPACE), then the pairs of the row; row_off [R + 1] and
 *   pairs (int32, DEVICE; pairs[p] = i NP + j < NP^2, ascending within a row) are the CSR of relative_position_index, which the caller builds and
 *   answers for.
 * afi_swin_patch_gather: out dense [N][ceil(H/4)][ceil(W/4)][48], channel 16 ci + 4 ky + kx = x[n][ci][4 oy + ky][4 ox + kx] of the dense NCHW
 *   x [N][3][H][W], zero outside it: PatchEmbed's conv as a 1x1 over patches, in the order of proj.weight.reshape(C, 48).
 * afi_swin_scale_add: out = a + s[n] b over dense [N][per_image] tensors (DropPath; s [N] on the device); a NULL: out = s[n] b; out may be a or b;
 *   per_image % 4 == 0. */
int afi_swin_layernorm_bwd_vecs(int Ct);
long long afi_swin_layernorm_bwd_ws_floats(int N, int H, int W, int C, int merge);
int afi_swin_layernorm_bwd(afi_view_t x, int N, int H, int W, int C, const float* gamma, float eps, int merge, const float* dy, afi_view_t dx,
                           float beta, float* dgamma, float* dbeta, float* ws, long long ws_floats, void* stream);
int afi_swin_gelu_bwd(const float* x, const float* dy, float* dx, long long n, void* stream);
long long afi_swin_window_attn_bwd_ws_floats(int N, int H, int W, int C, int window);
long long afi_swin_window_attn_bwd_groups(int N, int H, int W, int C, int window);
int afi_swin_window_attn_bwd(afi_view_t qkv, afi_view_t dout, int N, int H, int W, int C, const float* qkv_bias, const float* bias_img, int window,
                             int shift, float* dqkv, float* ds_part, long long ds_floats, void* stream);
long long afi_swin_bias_table_bwd_ws_floats(int heads, int window);
int afi_swin_bias_table_bwd(const float* ds_part, int nparts, int heads, int window, const int* row_off, const int* pairs, int R, float* dtable,
                            float* ws, long long ws_floats, void* stream);
int afi_swin_patch_gather(const float* x, int N, int H, int W, float* out, void* stream);
int afi_swin_scale_add(const float* a, const float* b, const float* s, int N, long long per_image, float* out, void* stream);

/* ------------------------------------------------------------------ frozen RPN proposal generator: selection (afigan_amd/rpn.py)
 * detectron2 v0.1.1's RPN at inference, after its head (which runs on afi_conv3x3_wino_infer / afi_conv3x3_fwd and one afi_conv1x1_fwd): per level
 * top-k, decode + clip + size test, greedy NMS; then the cross-level merge.  Anchor i of a level is (y W + x) A + a: cell anchor a shifted by
 * (x, y) * stride; no anchor tensor exists.  A <= 16, k <= 1024 per level, H W A < 2^22 - 1, at most 8 levels, N <= 65535 (AFI_ERR_UNSUPPORTED /
 * AFI_ERR_BAD_ARG otherwise).  Lists of one level are rows of `ld` elements (ld >= k), so the levels of an image can sit side by side in one
 * [N][sum k] buffer -- the layout afi_rpn_merge reads.  No entry point synchronises with the host; all results are bit-identical between runs.
 * afi_rpn_topk: logits = channels 0 .. A-1 of the view [N][H][W][.] (4-byte aligned is enough).  vals / idx [n][j], j < k <= H W A: the k highest
 *   logits of image n, by (logit descending, anchor index ascending) -- equal logits, -0 and +0 included, go in index order inside the list and
 *   at the cut; a NaN ranks below every number.  ws: afi_rpn_topk_ws_floats(N, H, W, A) floats, 8-byte aligned (0: none needed; -1: unsupported).
 * afi_rpn_decode: deltas = the view whose channel 4 a + c is coordinate c of anchor a's delta; cell_anchors [A][4] (device), image_hw [N][2]
 *   (device, fp32: the un-padded height, width).  boxes [n][j][4] = clip(Box2BoxTransform(wx, wy, ww, wh).apply_deltas, dw / dh clamped from
 *   above at scale_clamp), evaluated in fp64 from the fp32 inputs and rounded once; valid [n][j] = (x2 - x1 > min_size && y2 - y1 > min_size) on
 *   the stored fp32 box.  An index outside [0, H W A) gives a zero box, valid 0.
 * afi_rpn_nms: boxes [n][j][4], valid [n][j] in list order; keep [n][j] = 1 for a valid box no earlier kept box of the list overlaps with
 *   inter / (area_a + area_b - inter) > thresh (fp32, in that form).  k = 0 is accepted and launches nothing.
 * afi_rpn_merge: boxes [N][K][4], vals / keep [N][K], K = level_off[L]; level l is columns [level_off[l], level_off[l+1]) (level_off: HOST array
 *   of L + 1 ints, level_off[0] = 0), each level in afi_rpn_topk's order.  Output: the kept entries by (logit descending, level, rank), the first
 *   post_k of them: out_boxes [N][post_k][4], out_logits [N][post_k], counts [N]; rows from counts[n] on are zero. */
long long afi_rpn_topk_ws_floats(int N, int H, int W, int A);
int afi_rpn_topk(afi_view_t logits, int N, int H, int W, int A, int k, float* vals, int* idx, long long ld, float* ws, long long ws_floats,
                 void* stream);
int afi_rpn_decode(afi_view_t deltas, int N, int H, int W, int A, const float* cell_anchors, int stride, const int* idx, int k, long long ld,
                   const float* image_hw, float wx, float wy, float ww, float wh, double scale_clamp, float min_size, float* boxes, int* valid,
                   void* stream);
int afi_rpn_nms(const float* boxes, const int* valid, int N, int k, long long ld, float thresh, int* keep, void* stream);
int afi_rpn_merge(const float* boxes, const float* vals, const int* keep, int N, int L, const int* level_off, int post_k, float* out_boxes,
                  float* out_logits, int* counts, void* stream);

/* The wide forms of the three selection stages: per-level lists of up to 4096 entries (the reference's training configs set
 * PRE_NMS_TOPK_TRAIN 2000).  Same rules, layouts, status codes and determinism as the entry points above; no host synchronisation.
 * afi_rpn_topk_wide: afi_rpn_topk for 1024 < k <= 4096, k <= H W A (k <= 1024 is afi_rpn_topk's: AFI_ERR_UNSUPPORTED here, as is k > 4096).
 *   ws: afi_rpn_topk_wide_ws_floats(N, H, W, A) floats, 8-byte aligned (0: none needed; -1: unsupported) -- the size afi_rpn_topk needs.
 * afi_rpn_nms_wide: afi_rpn_nms for 0 <= k <= 4096 with the suppression bit matrix in ws: afi_rpn_nms_wide_ws_floats(N, k) =
 *   2 N k ceil(k / 64) floats, 8-byte aligned (-1: k > 4096).  The workspace need not be initialised: only words written by the call are read.
 *   For k <= 1024 the keep set is afi_rpn_nms's.
 * afi_rpn_merge_wide: afi_rpn_merge with levels of up to 4096 entries and level_off[L] <= 20480 (5 x 4096: the keys and positions of all
 *   levels are held in LDS) -- AFI_ERR_UNSUPPORTED above either. */
long long afi_rpn_topk_wide_ws_floats(int N, int H, int W, int A);
int afi_rpn_topk_wide(afi_view_t logits, int N, int H, int W, int A, int k, float* vals, int* idx, long long ld, float* ws, long long ws_floats,
                      void* stream);
long long afi_rpn_nms_wide_ws_floats(int N, int k);
int afi_rpn_nms_wide(const float* boxes, const int* valid, int N, int k, long long ld, float thresh, int* keep, float* ws, long long ws_floats,
                     void* stream);
int afi_rpn_merge_wide(const float* boxes, const float* vals, const int* keep, int N, int L, const int* level_off, int post_k, float* out_boxes,
                       float* out_logits, int* counts, void* stream);

/* ------------------------------------------------------------------ RPN training: labels, sampling, losses (afigan_amd/rpn.py: RPN.losses)
 * detectron2 v0.1.1's RPNOutputs._get_ground_truth (Matcher with low-quality matches), subsample_labels, Box2BoxTransform.get_deltas and
 * rpn_losses.  The levels of an image are concatenated in the order given: level_hw = HOST array {H_0, W_0, H_1, ...}, strides = HOST array of L
 * ints, cell_anchors = DEVICE [L][A][4]; global anchor index = the level's offset + (y W + x) A + a, the anchor box cell anchor a + (x, y) * stride
 * (one fp32 addition per coordinate).  R = sum H_l W_l A <= 2^22, A <= 16, L <= 8, N <= 65535.  Ground truth: gt [N][Gmax][4] fp32 (x1, y1, x2, y2)
 * with counts [N] (device int32; counts[n] is clamped to 0 .. Gmax), Gmax <= 1024.  No host synchronisation; bit-identical between runs.
 * afi_rpn_match: IoU in fp32, every operation rounded once (area = (x2 - x1)(y2 - y1), w = max(min(x2) - max(x1), 0), inter = w h,
 *   iou = inter > 0 ? inter / (area_gt + area_anchor - inter) : 0).  matched_idx [N][R] = the lowest box index that reaches the anchor's maximum
 *   IoU; labels [N][R] (int8) = 0 below t0, -1 in [t0, t1), 1 from t1 up; then label 1 for every anchor whose IoU with a box equals that box's
 *   maximum over all anchors (a box that overlaps nothing has maximum 0 and promotes every anchor with IoU 0: the reference's behaviour).
 *   counts[n] = 0: every label 0, matched_idx 0.  ws: N * Gmax floats.
 * afi_rpn_sample: keys [N][R] (32 bits each, compared unsigned).  num_pos = min(#label 1, num_pos_max), num_neg = min(#label 0,
 *   batch_per_image - num_pos): the num_pos positives and num_neg negatives with the smallest (key, anchor index) keep their label in labels_out
 *   (which must not be labels), every other label becomes -1.  sampled_idx [N][batch_per_image]: the sampled positives in ascending anchor
 *   index, then the negatives likewise, then -1; n_pos / n_neg [N].  batch_per_image <= 4096.
 * afi_rpn_loss: heads / grads = HOST arrays of L pixel-major views [N][H_l][W_l][>= 5 A]: channel a the logit, A + 4 a + c the deltas.  Over the
 *   sampled anchors: objectness max(z, 0) - z t + log1p(exp(-|z|)) (t = 1 for the first n_pos entries of an image's list), and for the positives
 *   smooth L1 (beta; |d| when beta < 1e-5) of delta - get_deltas(anchor, gt[matched_idx]) with weights (wx, wy, ww, wh), the target evaluated in
 *   fp64 and rounded once; terms in fp32, sums in fp64.  loss[0] = scale_cls * sum, loss[1] = scale_loc * sum (device fp32); grads receives
 *   d loss[0] / d logit and d loss[1] / d delta at the sampled anchors and is not touched elsewhere (the caller zero-fills it). */
int afi_rpn_match(const int* level_hw, const int* strides, int L, int A, const float* cell_anchors, int N, const float* gt, const int* counts,
                  int Gmax, float t0, float t1, signed char* labels, int* matched_idx, float* ws, long long ws_floats, void* stream);
int afi_rpn_sample(const signed char* labels, const unsigned int* keys, int N, long long R, int batch_per_image, int num_pos_max,
                   signed char* labels_out, int* sampled_idx, int* n_pos, int* n_neg, void* stream);
int afi_rpn_loss(const afi_view_t* heads, const afi_view_t* grads, const int* level_hw, const int* strides, int L, int A,
                 const float* cell_anchors, int N, const float* gt, int Gmax, const int* matched_idx, const int* sampled_idx, int batch_per_image,
                 const int* n_pos, const int* n_neg, float wx, float wy, float ww, float wh, float beta, double scale_cls, double scale_loc,
                 float* loss, void* stream);

/* ------------------------------------------------------------------ frozen box branch of StandardROIHeads (afigan_amd/roi_heads.py)
 * detectron2 v0.1.1's ROIPooler (ROIAlignV2, aligned = True) and fast_rcnn_inference; the box head's FCs and the predictor between them run on
 * afi_conv1x1_fwd over the R = N P rows as pixels.  Boxes of an image are rows of a padded [N][P][4] list with counts[N] (device int32): the
 * layout afi_rpn_merge writes.  No entry point synchronises with the host or uses atomics of its own (afi_roi_candidates runs afi_rpn_topk, whose
 * integer atomics only count); every result is bit-identical between runs.  N <= 65535 (AFI_ERR_BAD_ARG / AFI_ERR_UNSUPPORTED otherwise).
 * afi_roi_align: levels = HOST array of L <= 8 pixel-major views [N][H_l][W_l][C], level_hw = HOST array {H_0, W_0, H_1, ...}; level l has
 *   stride 2^(min_level + l).  C % 4 == 0, views 16-byte aligned with strides multiples of 4, 1 <= S <= 14, sampling_ratio >= 0.  out
 *   [N P][S][S][C] dense (pixel-major [R, C, S, S]); rows j >= counts[n] are zero.  Per box, in fp64 from the fp32 box, nothing stored:
 *   level = clamp(floor(4 + log2(sqrt(area) / 224)), min_level, min_level + L - 1), a zero or negative area (NaN too) at min_level;
 *   scale = 2^-level, start = x1 scale - 0.5, roi_w = (x2 - x1) scale, bin = roi_w / S, grid = sampling_ratio if > 0 else ceil(roi / S) per axis;
 *   sample (iy, ix) of bin (ph, pw) at start + p bin + (i + 0.5) bin / grid; bilinear as detectron2's bilinear_interpolate (zero outside
 *   [-1, H] x [-1, W], clamped at 0, y_low >= H - 1 collapses onto the last row); output = sum / max(grid_h grid_w, 1).  The four weights are
 *   rounded to fp32 and the sum is accumulated in fp32.  A box with a non-positive side gives zeros under either grid rule: with the adaptive grid
 *   that is detectron2's own result (no samples, count max(0, 1)), and the same reading is applied to a fixed sampling_ratio.
 * afi_roi_scores_boxes: pred [N P][ld_pred]: columns 0..K the class logits (background = column K), then 4 K (agnostic 0) or 4 (agnostic 1) box
 *   deltas.  scores [N][P][K] = softmax over the K + 1 logits without the background column, boxes [N][P][Kb][4] (Kb = K, or 1 when agnostic) =
 *   clip(Box2BoxTransform(wx, wy, ww, wh).apply_deltas(proposal), dw / dh clamped from above at scale_clamp), both evaluated in fp64 from the
 *   fp32 inputs and rounded once; no size test.  Rows j >= counts[n]: scores -inf, boxes zero.  A row with a NaN logit scores NaN.  K <= 1024.
 * afi_roi_cascade_stage: one stage of CascadeROIHeads.  s and boxes [N][P][4] are afi_roi_scores_boxes' with agnostic = 1, bit for bit (s = -inf
 *   past counts[n], NaN for a row with a NaN logit).  scores [N][P][K] = prev_scores ? prev_scores + s : s, then, when out_scale != 1, that times
 *   out_scale: one fp32 operation each, never contracted.  prev_scores NULL: the first stage.  scores may be prev_scores itself (a lane reads its
 *   element before it writes it).  Rows past counts stay -inf for every prev_scores below +inf, NaN rows stay NaN; boxes are the clipped decode,
 *   the next stage's proposals and the last stage's detection boxes.  0 < out_scale < inf.  ld_pred >= K + 5.
 * afi_roi_candidates: the m = min(M, P K) highest scores of image n by (score descending, index r K + c ascending), NaN below every number:
 *   cand_scores / cand_idx / cand_cls / cand_valid [N][M], cand_boxes [N][M][4]; valid = score > score_thresh; entries m.. are (-inf, -1, -1, 0,
 *   zero box).  n_over[n] = the count of ALL scores of image n above score_thresh.  M <= 1024, P K < 2^22 - 1.  ws:
 *   afi_roi_candidates_ws_floats(N, P, K) floats, 8-byte aligned (0: none needed; -1: unsupported).
 * afi_roi_nms: afi_rpn_nms with classes: an earlier kept box suppresses a later one only when cls is equal and inter / (area_a + area_b - inter)
 *   > thresh, in fp32 in that form on the boxes as they are (torchvision's batched_nms shifts every class by a coordinate offset instead, which
 *   rounds the boxes; not done here).  k <= 1024, k = 0 launches nothing.
 * afi_roi_pick: the first D <= 1024 kept candidates in list order: out_boxes [N][D][4], out_scores [N][D], out_classes [N][D] (int32), counts [N],
 *   zero past the count; truncated[n] = (n_over[n] > M && kept < D), the one case in which cutting the list at M can change the result. */
int afi_roi_align(const afi_view_t* levels, const int* level_hw, int L, int min_level, int N, int C, const float* boxes, const int* counts, int P,
                  int S, int sampling_ratio, float* out, void* stream);
int afi_roi_scores_boxes(const float* pred, long long ld_pred, int N, int P, int K, int agnostic, const float* proposals, const int* counts,
                         const float* image_hw, float wx, float wy, float ww, float wh, double scale_clamp, float* scores, float* boxes,
                         void* stream);
int afi_roi_cascade_stage(const float* pred, long long ld_pred, int N, int P, int K, const float* proposals, const int* counts,
                          const float* image_hw, float wx, float wy, float ww, float wh, double scale_clamp, const float* prev_scores,
                          float out_scale, float* scores, float* boxes, void* stream);
long long afi_roi_candidates_ws_floats(int N, int P, int K);
int afi_roi_candidates(const float* scores, const float* boxes, int N, int P, int K, int agnostic, float score_thresh, int M, float* cand_scores,
                       int* cand_idx, float* cand_boxes, int* cand_cls, int* cand_valid, int* n_over, float* ws, long long ws_floats,
                       void* stream);
int afi_roi_nms(const float* boxes, const int* cls, const int* valid, int N, int k, long long ld, float thresh, int* keep, void* stream);
int afi_roi_pick(const float* cand_boxes, const float* cand_scores, const int* cand_cls, const int* keep, const int* n_over, int N, int M, int D,
                 float* out_boxes, float* out_scores, int* out_classes, int* counts, int* truncated, void* stream);

/* ------------------------------------------------------------------ box branch of StandardROIHeads in training (roi_heads.py: StandardROIHeads.losses)
 * detectron2 v0.1.1's ROIHeads.label_and_sample_proposals, Box2BoxTransform.get_deltas, FastRCNNOutputs.softmax_cross_entropy_loss and
 * smooth_l1_loss, and the backward of afi_roi_align.  Proposals [N][P][4] with counts_p [N], ground truth gt [N][Gmax][4] (Gmax <= 1024) with
 * gt_classes [N][Gmax] (int32) and counts_g [N] (device int32, clamped to 0 .. P / Gmax).  The candidates of image n are one padded list of
 * R = P + Gmax entries: its counts_p[n] proposals, then (append_gt != 0) its counts_g[n] boxes, then padding.  The sample is afi_rpn_sample on
 * the labels with this R.  No host synchronisation, no float atomics; bit-identical between runs.
 * afi_roi_label: IoU as afi_rpn_match states it; matched_idx [N][R] = the lowest box index that reaches the candidate's maximum IoU, labels
 *   [N][R] (int8) = 1 from iou_thresh up, 0 below, -1 for padding; no low-quality matches.  counts_g[n] = 0: label 0 and matched_idx 0 on every
 *   candidate.
 * afi_roi_gather_samples: from sampled_idx [N][B], n_pos, n_neg (afi_rpn_sample's, B = batch_per_image): boxes [N][B][4], counts [N] = n_pos +
 *   n_neg, classes [N][B] (int32: gt_classes[matched_idx] for the first n_pos rows, K for the other sampled rows, -1 past the count), gt_boxes
 *   [N][B][4] (gt[matched_idx] of every sampled row; zeros when the image has no box and past the count).
 * afi_roi_box_loss: pred [N B][ld_pred] in afi_roi_scores_boxes' layout (K + 1 logits, background at K, then 4 K or 4 deltas).  Over the rows
 *   below counts: cross-entropy logsumexp(z) - z[class] in fp64; on rows with class < K smooth L1 (beta; |d| when beta < 1e-5) in fp32 of the
 *   four deltas of the row's class (columns K + 1 .. K + 4 when agnostic) minus get_deltas(box, gt_box) with weights (wx, wy, ww, wh), the
 *   target in fp64 rounded once.  Both sums in fp64 in a fixed order; loss[0], loss[1] (device fp32) = the sums / Rtot, Rtot = sum of counts,
 *   formed on the device (0: both losses and the whole gradient are zero).  dpred [N B][ld_pred] (not pred) is written completely:
 *   (softmax - onehot) / Rtot in fp64 rounded once, sign(d) or d / beta clamped to +-1 times fp32(1 / Rtot), zero everywhere else.
 *   ws: afi_roi_box_loss_ws_floats() floats, 8-byte aligned.
 * afi_roi_align_bwd: dpooled [N B][S][S][C] -> grads = HOST array of L pixel-major views [N][H_l][W_l][C], each written completely (zero where
 *   no box reaches).  Level, grid, inside test, clamp at 0 and the last-row collapse are afi_roi_align's fp64 expressions; per box and axis the
 *   1-D weights of a bin's samples on a pixel are summed in fp64 in sample order (W_y also divided by max(grid_h grid_w, 1)) and rounded to fp32
 *   once, and grad[y][x][c] = sum over (box, ph, pw) in that order of fp32(W_y W_x) * g[ph][pw][c] by fmaf.  One block owns an 8 x 8 tile of a
 *   level of an image.  ws: afi_roi_align_bwd_ws_floats(N, batch_per_image) floats, 16-byte aligned. */
int afi_roi_label(const float* proposals, const int* counts_p, int N, int P, const float* gt, const int* counts_g, int Gmax, int append_gt,
                  float iou_thresh, signed char* labels, int* matched_idx, void* stream);
int afi_roi_gather_samples(const float* proposals, const int* counts_p, int N, int P, const float* gt, const int* gt_classes, const int* counts_g,
                           int Gmax, int append_gt, const int* matched_idx, const int* sampled_idx, const int* n_pos, const int* n_neg,
                           int batch_per_image, int K, float* boxes, int* counts, int* classes, float* gt_boxes, void* stream);
long long afi_roi_box_loss_ws_floats(void);
int afi_roi_box_loss(const float* pred, long long ld_pred, int N, int batch_per_image, int K, int agnostic, const float* boxes, const int* counts,
                     const int* gt_classes, const float* gt_boxes, float wx, float wy, float ww, float wh, float beta, float* loss, float* dpred,
                     float* ws, long long ws_floats, void* stream);
long long afi_roi_align_bwd_ws_floats(int N, int batch_per_image);
int afi_roi_align_bwd(const float* dpooled, const afi_view_t* grads, const int* level_hw, int L, int min_level, int N, int C, const float* boxes,
                      const int* counts, int batch_per_image, int S, int sampling_ratio, float* ws, long long ws_floats, void* stream);

/* ------------------------------------------------------------------ CascadeROIHeads in training (csrc/cascade_train.hip)
 * The two passes of a cascade stage in training that are specific to the padded [N][B] row lists with device-side counts.  No host
 * synchronisation, no atomics; every result is bit-identical between runs and every output is written completely.
 * afi_roi_cascade_relabel: detectron2 v0.1.1's _create_proposals_from_boxes + _match_and_label_boxes.  pred [N B][ld_pred], proposals [N][B][4],
 *   counts [N], image_hw, the four weights and scale_clamp as afi_roi_cascade_stage takes them: rows below counts[n] are decoded and clipped by
 *   the device function that kernel instantiates, so the boxes are its boxes bit for bit.  A row is kept when, in fp32 on the clipped box,
 *   x2 - x1 > 0 and y2 - y1 > 0 (Boxes.nonempty(); a NaN box is dropped).  Kept rows are written in their original order: boxes [N][B][4],
 *   src [N][B] = the input row, counts_out [N] = their number.  Each is matched to gt [N][Gmax][4] (counts_g [N]) as afi_roi_label states it:
 *   matched_idx [N][B] = the lowest ground-truth index that reaches the maximum IoU, label 1 from iou_thresh up, no low-quality matches;
 *   classes [N][B] (int32) = gt_classes[matched] where the label is 1, K otherwise; gt_boxes [N][B][4] = gt[matched] on every kept row.
 *   counts_g[n] = 0: class K, matched_idx 0 and a zero gt_boxes on every kept row.  Past counts_out[n]: boxes and gt_boxes zero, classes -1,
 *   src -1, matched_idx 0.  B <= 4096, Gmax <= 1024, K <= 1024 (AFI_ERR_UNSUPPORTED), ld_pred >= K + 5; boxes and gt_boxes 16-byte aligned.
 * afi_roi_bn_*: train-mode BatchNorm (+ ReLU) over x [N B][P1][C] (dense, pixel-major: P1 pixels per list row) in which row n B + j exists iff
 *   j < counts[n] (counts clamped to 0 .. B).  Pn = P1 sum(min(counts, B)) is formed on the device.  Padding rows of x, g and y are never read
 *   into a result.  C % 4 == 0, every pointer 16-byte aligned, N <= 1024, B <= 4096 and N B P1 C / 4 < 2^31 (AFI_ERR_UNSUPPORTED).  scratch: afi_reduce_scratch_floats(C) floats, 32-byte aligned.
 *   afi_roi_bn_stats           mean, invstd = 1 / sqrt(var + eps) and (optional) the biased variance over the Pn valid pixels, accumulated as
 *                              afi_bn_stats_ex does (fp64, shifted by the first valid pixel, rounded once); the running buffers (both or
 *                              neither) are updated with momentum, the variance unbiased over Pn, and num_batches_tracked += 1.  Pn == 0:
 *                              mean 0, invstd 1 / sqrt(eps), variance 0; the running buffers and the counter stay untouched.
 *   afi_roi_bn_relu_fwd        valid rows: y = max(0, ((x - mean) invstd) gamma + beta) with relu = 1, the plain affine with relu = 0, every
 *                              operation rounded on its own (afi_bn_apply_fwd's arithmetic); padding rows: y = 0 exactly.
 *   afi_roi_bn_relu_bwd_sums   sums2C[0..C) = sum g', sums2C[C..2C) = sum g' xhat over the valid rows, g' = g [y > 0] from the STORED y
 *                              (relu = 1; relu = 0: g' = g and y may be NULL), xhat = (x - mean) invstd; dbeta / dgamma (optional) += them.
 *   afi_roi_bn_relu_bwd_apply  valid rows: dx = gamma invstd (g' - s0 / Pn - xhat s1 / Pn); padding rows, and every row when Pn == 0: dx = 0.
 *                              dx may be g. */
int afi_roi_cascade_relabel(const float* pred, long long ld_pred, int N, int B, int K, const float* proposals, const int* counts,
                            const float* image_hw, float wx, float wy, float ww, float wh, double scale_clamp, const float* gt,
                            const int* gt_classes, const int* counts_g, int Gmax, float iou_thresh, float* boxes, int* counts_out, int* classes,
                            float* gt_boxes, int* src, int* matched_idx, void* stream);
int afi_roi_bn_stats(const float* x, const int* counts, int N, int B, int P1, int C, float eps, float momentum, float* mean, float* invstd,
                     float* var_biased_or_null, float* running_mean_or_null, float* running_var_or_null,
                     long long* num_batches_tracked_or_null, float* scratch, void* stream);
int afi_roi_bn_relu_fwd(const float* x, const int* counts, int N, int B, int P1, int C, const float* mean, const float* invstd,
                        const float* gamma, const float* beta, int relu, float* y, void* stream);
int afi_roi_bn_relu_bwd_sums(const float* g, const float* x, const float* y_or_null, const int* counts, int N, int B, int P1, int C,
                             const float* mean, const float* invstd, int relu, float* dgamma_or_null, float* dbeta_or_null, float* sums2C,
                             float* scratch, void* stream);
int afi_roi_bn_relu_bwd_apply(const float* g, const float* x, const float* y_or_null, const int* counts, int N, int B, int P1, int C,
                              const float* mean, const float* invstd, const float* gamma, const float* sums2C, int relu, float* dx,
                              void* stream);

/* ------------------------------------------------------------------ frozen mask branch of StandardROIHeads (afigan_amd/roi_heads.py)
 * detectron2 v0.1.1's mask_rcnn_inference and paste_masks_in_image.  The mask pooler is afi_roi_align on the padded detections, the head's 3x3
 * convs are the frozen conv dispatch, and the deconv (ConvTranspose2d kernel 2, stride 2) is one afi_conv1x1_fwd over a [4 Cout][Cin] weight
 * (row (2a + b) Cout + co = deconv.weight[ci][co][a][b]), whose dense output [R][S][S][4][C] holds phase 2a + b of input pixel (y, x) = output
 * pixel (2y + a, 2x + b).  No host synchronisation, no atomics; every result is bit-identical between runs.
 * afi_roi_mask_probs: h = that layout, R = N D rows; w [Km][C], bias [Km]; classes [N][D] (int32), counts [N].  probs [N D][2S][2S]:
 *   z = bias[c] + sum_k w[c][k] h[k] for the row's class c (0 when Km == 1) in fp32 (fmaf per lane in channel order, a fixed butterfly), then
 *   p = 1 / (1 + exp(-z)) in fp64 from the fp32 z, rounded once.  Rows d >= counts[n] and rows whose class is outside 0 .. Km - 1 are zero and
 *   read neither h nor w.  C % 4 == 0, 1 <= S <= 14, h and w 16-byte aligned, N <= 65535.
 * afi_mask_paste: probs [R][M][M], boxes [R][4] (x0, y0, x1, y1, fp32), out [R][H][W], one byte per pixel, 0 or 1.  For a pixel (y, x) whose
 *   centre lies inside the box (x0 <= x + 0.5 <= x1 and y0 <= y + 0.5 <= y1): gx = (x + 0.5 - x0) / (x1 - x0) 2 - 1, ix = ((gx + 1) M - 1) / 2
 *   (gy, iy likewise), in fp64 from the fp32 box, operation by operation; taps floor(ix), floor(ix) + 1 with weights 1 - frac, frac per axis, a
 *   tap outside 0 .. M - 1 contributing zero (grid_sample: bilinear, zeros padding, align_corners false); the four weights are rounded to fp32
 *   and v = fma(w11, m11, fma(w10, m10, fma(w01, m01, w00 m00))) in fp32 (y0x0, y0x1, y1x0, y1x1); out = v >= threshold.  Every other pixel
 *   is 0 -- detectron2 samples only a region around the boxes; at threshold 0.5 and probabilities <= 1 a pixel whose centre is outside its box
 *   cannot reach the threshold, so this equals sampling the whole image.  A box with a non-positive or NaN side gives zeros.  M <= 64,
 *   H <= 2097120; out may start at any byte.  R = 0 is accepted and launches nothing. */
int afi_roi_mask_probs(const float* h, const float* w, const float* bias, const int* classes, const int* counts, int N, int D, int C, int S, int Km,
                       float* probs, void* stream);
int afi_mask_paste(const float* probs, const float* boxes, int R, int M, int H, int W, float threshold, unsigned char* out, void* stream);

/* ------------------------------------------------------------------ pasted masks as COCO run-length starts (csrc/mask_rle.hip)
 * The mask afi_mask_paste would write, pixel for pixel (the same inside test, fp64 coordinate steps, fp32-rounded weights, fmaf order and
 * `>= threshold`), as the starts of its runs and without the image-size mask: only pixels inside a box are formed.  A mask [H][W] is read in
 * column-major order, j = x H + y, f[-1] = 0; a start is a j with f[j] != f[j - 1].  With the starts B_0 < ... < B_{m-1} of a detection, COCO's
 * counts are [B_0, B_1 - B_0, ..., H W - B_{m-1}] ([H W] for an empty mask).  A box with a non-positive or NaN side gives an empty mask, as in
 * afi_mask_paste; so does, by definition here, a box with a non-finite coordinate.
 * afi_mask_rle_ws_bytes: the workspace of one call pair: bits [R][ceil(H / 64)][W] (uint64, bit b of word k = row 64 k + b) and the per-column
 *   start counts [R][W] (int32); -1 for an unsupported shape.  Only the words and columns of each box's pixel extent are written and read.
 * afi_mask_rle_count: nstarts [R] (int32, device) = the number of starts of every detection; fills ws.
 * afi_mask_rle_emit: after the caller turned nstarts into exclusive offsets [R] (long long, device, in elements of starts): the starts of
 *   detection r, ascending, at starts[offsets[r] ..] (int32).  ws: unchanged since afi_mask_rle_count with the same boxes, R, H, W.
 * M <= 64, H W < 2^31, H <= 2097120; ws and offsets 8-byte aligned.  R = 0 is accepted and launches nothing.  No atomics, no host
 * synchronisation; bit-identical between runs. */
long long afi_mask_rle_ws_bytes(int R, int H, int W);
int afi_mask_rle_count(const float* probs, const float* boxes, int R, int M, int H, int W, float threshold, void* ws, long long ws_bytes,
                       int* nstarts, void* stream);
int afi_mask_rle_emit(const float* boxes, int R, int H, int W, const void* ws, long long ws_bytes, const long long* offsets, int* starts,
                      void* stream);

/* ------------------------------------------------------------------ COCO evaluation: IoU and greedy matching (csrc/coco_eval.hip)
 * pycocotools' COCOeval.computeIoU and evaluateImg for bbox and segm (afigan_amd/coco_eval.py accumulates on the host).  Work comes in groups,
 * one per (image, category): the D detections of a group (the caller sorted them by descending score, stably, and cut them, to 100 for COCO) and
 * its G ground truths in annotation order are rows dt_off[i] .. dt_off[i + 1] and gt_off[i] .. gt_off[i + 1] of the per-detection and per-GT
 * arrays, and its matrix [D][G], row-major, is iou_off[i] .. iou_off[i + 1] of the packed matrices: three device arrays of ngroups + 1 long long
 * with iou_off[i + 1] - iou_off[i] = D G; total = iou_off[ngroups] (the caller knows it).  Every pointer is a device pointer.  fp64 throughout,
 * operation by operation as written here (no contraction), so a numpy fp64 restatement gives the same bits.  No atomics, no host
 * synchronisation; bit-identical between runs.  ngroups = 0 or total = 0 is accepted and launches nothing.
 * afi_coco_box_iou: dt [total_d][4], gt [total_g][4] as (x, y, w, h), iscrowd [total_g] bytes.  w = min(dx + dw, gx + gw) - max(dx, gx), h
 *   likewise; w <= 0 or h <= 0 gives 0, else i = w h, u = crowd ? dw dh : dw dh + gw gh - i, iou = i / u.
 * Masks are ascending run starts (afi_mask_rle_emit's, rle.counts_from_starts' format; equal neighbours, i.e. empty runs, are allowed): mask m
 *   is starts[start_off[m] .. start_off[m + 1]) (start_off: nmask + 1 long long) on hw[m] = H W pixels (int32); pixels from an even-indexed start
 *   up to the next start (or H W) are set.
 * afi_coco_rle_area: area[m] = the number of set pixels (long long).
 * afi_coco_rle_iou: inter = the number of pixels set in both masks of a pair (a two-pointer merge, entered by a binary search at the first pixel
 *   where both masks have begun and left at the first where one has ended), u = crowd ? area(d) : area(d) + area(g) - inter,
 *   iou = u == 0 ? 0 : (double)inter / (double)u.  dt_area / gt_area: afi_coco_rle_area's.  A pair of masks with different H W gives -1 (both
 *   outputs).  inter (long long, packed like iou) may be NULL.
 * afi_coco_match: the greedy matching for A area ranges (area_rng [A][2] = lo, hi) x T thresholds (iou_thr [T]) per group; dt_area [total_d],
 *   gt_area [total_g] fp64.  gt_ignore [A][total_g] = iscrowd || area < lo || area > hi.  For each detection d in order: best = min(thr, 1 - 1e-10),
 *   m = -1; over the non-ignored GTs in order, then -- only while m is still -1 -- over the ignored ones: skip a GT already matched at this
 *   (a, t) unless it is a crowd; skip it if iou[d][g] < best; else best = iou[d][g], m = g (an equal IoU moves the match to the later GT).
 *   dt_match [A][T][total_d] (int32) = m, the GT's index inside its group, or -1; dt_ignore [A][T][total_d] = gt_ignore[a][m], or, unmatched,
 *   (dt_area < lo || dt_area > hi).  max_g: the caller's upper bound on the G of any group (it built the offsets); only when max_g > 64 is the
 *   kernel for groups of more than 64 GTs launched at all; a group with G > max_g is left unmatched (its outputs are not written);
 *   A max_g < 2^31 (AFI_ERR_UNSUPPORTED).  ws: afi_coco_match_ws_bytes(total_g, A, T) bytes (-1: unsupported, A T > 4096), read only after being
 *   written; a smaller ws_bytes is AFI_ERR_BAD_ARG. */
int afi_coco_box_iou(const double* dt, const double* gt, const unsigned char* iscrowd, const long long* dt_off, const long long* gt_off,
                     const long long* iou_off, int ngroups, long long total, double* iou, void* stream);
int afi_coco_rle_area(const int* starts, const long long* start_off, const int* hw, long long nmask, long long* area, void* stream);
int afi_coco_rle_iou(const int* dt_starts, const long long* dt_start_off, const int* dt_hw, const long long* dt_area, const int* gt_starts,
                     const long long* gt_start_off, const int* gt_hw, const long long* gt_area, const unsigned char* iscrowd,
                     const long long* dt_off, const long long* gt_off, const long long* iou_off, int ngroups, long long total, long long* inter,
                     double* iou, void* stream);
long long afi_coco_match_ws_bytes(long long total_g, int A, int T);
int afi_coco_match(const double* iou, const long long* dt_off, const long long* gt_off, const long long* iou_off, int ngroups,
                   const double* dt_area, const double* gt_area, const unsigned char* iscrowd, long long total_d, long long total_g,
                   const double* area_rng, int A, const double* iou_thr, int T, int max_g, int* dt_match, unsigned char* dt_ignore,
                   unsigned char* gt_ignore, void* ws, long long ws_bytes, void* stream);

/* ------------------------------------------------------------------ COCO polygons as run-length starts, and their decode (csrc/poly_rle.hip)
 * pycocotools' rleFrPoly, the union of one annotation's polygons (frPyObjects + merge) and decode, in the starts format above, so that
 * polygon ground truth feeds afi_coco_rle_area / afi_coco_rle_iou directly.  A polygon is k >= 1 vertices (x, y) on a canvas of H x W pixels;
 * all arithmetic is fp64, operation by operation as written (no contraction); (int) truncates toward zero:
 *   X[j] = (int)(5 x_j + .5), Y[j] likewise, X[k] = X[0].  Edge j runs from (xs, ys) = (X[j], Y[j]) to (xe, ye) = (X[j + 1], Y[j + 1]); dx = |xe - xs|,
 *   dy = |ye - ys|; flip = (dx >= dy && xs > xe) || (dx < dy && ys > ye) swaps the two ends; s = dx >= dy ? (double)(ye - ys) / dx :
 *   (double)(xe - xs) / dy; for d = 0 .. max(dx, dy), t = flip ? max(dx, dy) - d : d, the point is (u, v) = (t + xs, (int)(ys + s t + .5)) if
 *   dx >= dy, else ((int)(xs + s t + .5), t + ys); an edge with dx = dy = 0 is the one point (xs, ys).  For consecutive points p - 1, p of the
 *   list of all edges' points with u[p] != u[p - 1]: xd = u[p] < u[p - 1] ? u[p] : u[p] - 1, xd = (xd + .5) / 5 - .5, kept if xd is an integer in
 *   0 .. W - 1; yd = min(v[p], v[p - 1]), yd = (yd + .5) / 5 - .5, clamped to [0, H], yd = ceil(yd); the crossing is a = (int)xd H + (int)yd.
 *   The starts of a polygon are its crossings of odd multiplicity below H W, ascending.  A mask of several polygons is their union: the start of
 *   rank r in its polygon counts +1 (r even) or -1 (r odd), and a position is a start of the union iff the running depth is zero on exactly
 *   one side of the events at that position.  A mask without a polygon, or whose polygons give no start, is empty.
 * The batch: xy [V][2] (double), vert_off [P + 1] and poly_off [N + 1] (long long: the vertices of polygon p, the polygons of mask m), hw [N][2]
 *   = (H, W) of every mask (int32; masks of one call may differ in size; H W < 2^31 and |5 c + .5| < 2^30 for every coordinate c are the
 *   CALLER's to check, as is that every polygon has a vertex), cap_off [P + 1] (long long) = the exclusive prefix of a per-polygon bound on the
 *   crossings, sum over its edges of (dx / 5 + 2) with dx in upsampled units; cap_total = cap_off[P] < 2^31.  Every pointer is a device pointer.
 * afi_poly_rle_ws_bytes(cap_total): the workspace of one call pair (8-byte sort keys and int32 starts per bounded crossing); -1: unsupported.
 *   A smaller ws_bytes is AFI_ERR_BAD_ARG.  The workspace is read only after being written.
 * afi_poly_rle_count: nstarts [N] (int32) = the number of starts of every mask, -1 for a mask whose crossings exceed its capacity (nothing is
 *   written past a mask's slice).  One block per mask; a mask of at most AFI_POLY_RLE_LDS_CAP crossings is sorted in LDS, a larger one in its
 *   slice of the workspace.
 * afi_poly_rle_emit: after the caller scanned nstarts into start_off [N + 1] (long long): the starts of mask m, ascending, at
 *   starts[start_off[m] ..] (int32).  ws: unchanged since afi_poly_rle_count with the same poly_off, cap_off, N, cap_total.
 * afi_rle_decode: N masks of one common H x W as starts / start_off [N + 1]; out [N][H][W] bytes, row-major: pixel (y, x) = 1 iff the number of
 *   starts <= x H + y is odd, else 0; every byte is written.
 * N = 0 is accepted and launches nothing.  No atomics, no host synchronisation; bit-identical between runs. */
#define AFI_POLY_RLE_LDS_CAP 4096
long long afi_poly_rle_ws_bytes(long long cap_total);
int afi_poly_rle_count(const double* xy, const long long* vert_off, const long long* poly_off, const int* hw, const long long* cap_off, int N,
                       long long cap_total, void* ws, long long ws_bytes, int* nstarts, void* stream);
int afi_poly_rle_emit(const long long* poly_off, const long long* cap_off, int N, long long cap_total, const void* ws, long long ws_bytes,
                      const long long* start_off, int* starts, void* stream);
int afi_rle_decode(const int* starts, const long long* start_off, int N, int H, int W, unsigned char* out, void* stream);

/* ------------------------------------------------------------------ the mask branch of StandardROIHeads in training (csrc/mask_loss.hip)
 * detectron2 v0.1.1's mask_rcnn_loss restated.  The mask branch runs on the first Bf rows of every image of the box
 * branch's training list (afi_roi_gather_samples puts the n_pos positives first): boxes [N][batch_per_image][4], classes
 * [N][ld_classes], both read in place with their own row stride.  No float atomics, no host synchronisation; bit-identical between runs.
 * afi_mask_targets: targets [N][Bf][M][M] bytes (0 / 1, row-major), every byte written, and counts_fg [N] = n_pos clamped to 0 .. Bf.  Row j
 *   of image n is live when j < counts_fg[n], its sampled index i = sampled_idx[n][j] lies in 0 .. ld_matched - 1 and the image has
 *   G = clamp(counts_g[n], 0, Gmax) > 0 boxes; its instance is g = clamp(matched_idx[n][i], 0, G - 1) (afi_roi_gather_samples' rule), whose
 *   polygons are poly_off[n Gmax + g] .. poly_off[n Gmax + g + 1] of the batch format above (xy, vert_off [num_poly + 1], poly_off
 *   [N Gmax + 1]; offsets outside 0 .. num_poly / 0 .. num_vert give the empty mask).  From the row's fp32 box (x0, y0, x1, y1): w = x1 - x0,
 *   h = y1 - y0 in fp32; rw = (double)w < 0.1 ? (double)M / 0.1 : (double)((float)M / w) (a NaN w takes the fp32 quotient), rh likewise; every
 *   vertex becomes X = (x - (double)x0) rw, Y = (y - (double)y0) rh (one fp64 subtraction, one fp64 product, no contraction); the target is the
 *   union of the polygons on the M x M canvas by the rules above.  A row with a transformed coordinate c that is not finite or has
 *   |5 c + .5| >= 2^30 is zero (decided on the double; no out-of-range conversion is made), as is a row that is not live or has no polygon.
 *   M <= 28.
 * afi_mask_loss: h = afi_roi_mask_probs' layout [N D][S][S][4][C] with D = Bf, w [Km][C], bias [Km], targets [N D][2S][2S].  For a live row
 *   (d < clamp(counts_fg[n], 0, D), class c = classes[n][d] in 0 .. Km - 1; c = 0 when Km == 1) and output pixel p: z = afi_roi_mask_probs'
 *   fp32 logit; term = max(z, 0) - z t + log1p(exp(-|z|)) and dz = (1 / (1 + exp(-z)) - t) / Mtot in fp64 from the fp32 z, dz rounded once.
 *   Mtot = 4 S S sum of the clamped counts, formed on the device.  loss[0] (device fp32) = sum of the terms (fp64, fixed order) / Mtot, rounded
 *   once; 0 when Mtot = 0.  dz [N D][S][S][4] (h's pixel order) is written completely, zero on rows that are not live.
 *   ws: afi_mask_loss_ws_floats(N, D, C, S) floats, 8-byte aligned.
 * afi_mask_pred_bwd: dh (h's layout, not h) = dz w[c][k] (h > 0 ? 1 : 0), one fp32 product, written completely (zero on rows that are not
 *   live); dW [Km][C], db [Km]: per live row and pixel part the fp32 fmaf sums of dz h[k] and the fp32 sum of dz in pixel order, then per class
 *   the partials of its rows added in (row, part) order in fp64 and rounded once; a class without a row gets zeros.  dz may have been scaled
 *   by the caller.  C <= 1024, N D <= 65535.  ws: afi_mask_pred_bwd_ws_floats(N, D, C) floats, 16-byte aligned. */
int afi_mask_targets(const double* xy, const long long* vert_off, const long long* poly_off, long long num_poly, long long num_vert,
                     const float* boxes, const int* sampled_idx, int N, int batch_per_image, const int* matched_idx, int ld_matched,
                     const int* counts_g, int Gmax, const int* n_pos, int Bf, int M, unsigned char* targets, int* counts_fg, void* stream);
long long afi_mask_loss_ws_floats(int N, int D, int C, int S);
int afi_mask_loss(const float* h, const float* w, const float* bias, const int* classes, int ld_classes, const int* counts_fg,
                  const unsigned char* targets, int N, int D, int C, int S, int Km, float* loss, float* dz, float* ws, long long ws_floats,
                  void* stream);
long long afi_mask_pred_bwd_ws_floats(int N, int D, int C);
int afi_mask_pred_bwd(const float* h, const float* dz, const float* w, const int* classes, int ld_classes, const int* counts_fg, int N, int D,
                      int C, int S, int Km, float* dh, float* dW, float* db, float* ws, long long ws_floats, void* stream);

/* ------------------------------------------------------------------ measurement support (bench.py)
 * When enabled, every MFMA GEMM launch is bracketed by two hipEvents recorded on the launch stream.
 * afi_profile_get(kind, out): out[0] launches, out[1] total ms, out[2] total algorithmic FLOP of that kernel since
 * the last afi_profile_enable(1).  One switch for the process (the launchers see streams, not contexts); its records are kept under a mutex, so
 * launches of several threads may be bracketed at once; the readers are meant for one benchmarking thread after a device synchronisation.
 * Off unless enabled: bench.py enables it for a separate pass of the same steps behind its timed region, not inside it (bench.py --profile-timed does). */
int afi_profile_enable(int on);
int afi_profile_num_kinds(void);
const char* afi_profile_kind_name(int kind);
int afi_profile_get(int kind, double* out3);
/* one CSV line per recorded launch (kind, GEMM rows, columns, K, split-K factor, ms, TFLOP/s) */
int afi_profile_dump(const char* path);

/* ------------------------------------------------------------------ diagnostics (host-only, no GPU needed)
 * The ownership the stream-K cut of the grouped small-map weight gradients (afi_generator_bwd on maps of <= 3000 pixels) gives every dW
 * tile: problem i has tiles[i] tiles of ceil(pixels[i] / 32) pixel stages; bpc = resident blocks per CU the runs are cut for (3).
 * Per tile (numbered problem-major): stored = runs that store it whole, added = runs that add to it by atomics, stages = stages covered.
 * A valid plan has (stored, added) = (1, 0) or (0, >= 2) and full stage coverage for every tile; tests/test_cabi.py checks exactly that. */
int afi_debug_wgrad_sk_plan(const long long* pixels, const int* tiles, int nprob, int bpc, int* stored, int* added, int* stages);
/* (GPU) The bf16x6 weight image of a conv-transpose weight W [Cin][Cout][6][6] built the two ways the library knows, for a byte comparison
 * (tests/test_gpu_ops.py): `direct` straight from W's own layout by the LDS-tiled blocks that ride in the small-map image launch, together
 * with the packed fp32 form `pack_ride` [4 Cout][9][Cin] written by further blocks of that launch; `via_pack` from the packed form
 * `pack_ref` made by the stand-alone pack kernel, through the generic image job.  mode 0: the forward's image (4 Cout columns, K = Cin),
 * mode 1: the data gradient's (Cin columns, K = (Cout chunk, phase, tap)).  Returns the image size in bytes through *bytes (buffers may be
 * null to query it).  Cin, Cout multiples of 32. */
int afi_debug_wk6_convT_images(const float* W, int Cin, int Cout, int mode, void* direct, float* pack_ride, void* via_pack, float* pack_ref,
                               long long* bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AFIGAN_HIP_H */
