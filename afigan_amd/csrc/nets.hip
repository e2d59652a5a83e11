// C-ABI of libafigan_hip.so: per-op entry points and the whole-network forward / backward sequencing of the
// AF interpolator (generator_rdb.py:73-130) and the feature-patch discriminator
// (feature_patch_discriminator.py:16-55).  Host code only: it fills kernel parameter blocks and launches the
// kernels of igemm.hip / elementwise.hip on the caller's stream.  No allocation, no synchronisation.
#include <string.h>
#include <stdlib.h>

#include "../../include/afigan_hip.h"
#include "afi_common.h"
#include "afi_launch.h"
#include <initializer_list>
#include <new>


// ---- the caller-owned context (include/afigan_hip.h: afi_ctx_t): every piece of state that outlives one call lives here, nothing is
//      process-global.  One context serves one stream at a time; two engines in one process use two contexts.
#include <vector>
namespace {
struct SideStream {                                        // fork/join target of the backward passes of small / mid-size maps
    hipStream_t side = nullptr;
    std::vector<hipEvent_t> ring;
    size_t next = 0;
    bool init() {
        if (side) return true;
        if (hipStreamCreateWithFlags(&side, hipStreamNonBlocking) != hipSuccess) { side = nullptr; return false; }
        ring.resize(128);
        for (auto& e : ring)
            if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return false;
        return true;
    }
    void destroy() {
        for (auto& e : ring) if (e) (void)hipEventDestroy(e);
        ring.clear();
        if (side) (void)hipStreamDestroy(side);
        side = nullptr;
    }
    hipEvent_t ev() { hipEvent_t e = ring[next]; next = (next + 1) % ring.size(); return e; }
};
struct WinoWeightCache {
    float* buf = nullptr;
    long long floats = 0, used = 0;
    struct Entry { const float* w; int f4, mode, O, I; long long off; } e[128];
    int n = 0;
};
struct WinoWgradAccum {
    float* buf = nullptr;
    long long floats = 0, used = 0;
    struct Entry { float* dw; int f4, O, I; float alpha; long long off; } e[64];
    int n = 0;
};
}  // namespace
// Per-context options (afi_ctx_set_option; include/afigan_hip.h lists them).  Nothing in the library reads the environment: a choice that
// changes numerics or scheduling is made by the caller, per context, and can be changed between calls.  Context-less calls use the defaults.
struct AfiOptions { long long v[AFI_OPT_COUNT]; };
#ifndef AFI_DEFAULT_LOCAL_SUMS
#define AFI_DEFAULT_LOCAL_SUMS 12
#endif
#ifndef AFI_DEFAULT_F4_FORWARD
// Blocks 1 and 2, with the k-step-local sums of AFI_OPT_F16_LOCAL_SUMS in both.  Round 6 decided it from profiles/r06/dflip_p{2,3}_*_6seeds_local_sums.txt
// (D fwd+bwd against fp64 at P2 and P3, six seeds each): the default is the largest block set whose dx AND worst-parameter-gradient deviation stay
// below torch's own fp32 ops on the same inputs.  Plain summation order: = 8 does (P3 0.97e-3 / 1.31e-3 against torch 1.15e-3 / 1.54e-3; P2 1.14e-3 /
// 1.51e-3 against 1.21e-3 / 1.54e-3), = 12 -- round 5's default -- does not (1.27e-3 / 1.73e-3; 1.45e-3 / 1.91e-3) and triples the LeakyReLU mask
// flips at 2x50x84.  With the local sums = 12 is BELOW = 8 (P3 0.88e-3 / 1.26e-3; P2 1.04e-3 / 1.33e-3) for 2.7 ms less per step; = 1 still fails
// (block 0's planes are not pre-split: no local sums there).  tests/test_gpu_d_parity.py enforces the bar.  (A/B builds: -DAFI_DEFAULT_F4_FORWARD=..)
#define AFI_DEFAULT_F4_FORWARD 12
#endif
static const AfiOptions kDefaultOptions = {{/*WINOGRAD*/ 1, /*F4_BACKWARD*/ 1, /*F4_FORWARD*/ AFI_DEFAULT_F4_FORWARD, /*BN_STATS_FP64*/ 1, /*D_WINOGRAD_MIN_PIXELS*/ 1024,
                                            /*G_WINOGRAD_MIN_PIXELS*/ 2048, /*G_SMALLMAP_MAX_PIXELS*/ 2048, /*G_GROUPED_WGRAD_MAX_PIXELS*/ 3000,
                                            /*G_BATCH_GROWTH_GRADS*/ 1, /*G_SMALLMAP6_MAX_PIXELS*/ 4096, /*DETERMINISTIC*/ 0, /*F16_PRESPLIT*/ 1, /*F16_NT256_MIN_TILES*/ 512,
                                            /*F16_LOCAL_SUMS*/ AFI_DEFAULT_LOCAL_SUMS, /*D_FUSE_TAIL*/ 1}};
struct afi_ctx {
    int device = -1;                                       // the device the context was created on; calls on another one are refused
    float* op_scratch = nullptr; long long op_scratch_floats = 0;
    int dtype = AFI_DTYPE_DEFAULT;                         // arithmetic of the Winograd-domain GEMMs (afi_ctx_set_compute_dtype)
    AfiOptions opt = kDefaultOptions;
    WinoWeightCache wcache;
    WinoWgradAccum wgacc;
    SideStream side;
    // f16x3: the zero-filled slots the Winograd transforms raise to their source tensor's largest magnitude (afi_gemm_f16.h) are taken from
    // the last kWinoAmaxFloats of the Winograd scratch a call works in, one memset per public call and scratch region (two regions: the
    // backward passes keep a second scratch for the weight gradients) instead of one per convolution.  AFI_CTX_CHECK, which every public
    // entry point passes, forgets both.
    struct AmaxPool { float* p = nullptr; int next = 0; } amax[2];
};
static inline long long afi_opt(const afi_ctx* cx, int o) { return cx ? cx->opt.v[o] : kDefaultOptions.v[o]; }
static inline int afi_default_dtype() { return AFI_DTYPE_DEFAULT; }

static inline bool afi_dtype_ok(int d) { return d == AFI_DTYPE_F32 || d == AFI_DTYPE_BF16 || d == AFI_DTYPE_F16X3 || d == AFI_DTYPE_BF16X3 || d == AFI_DTYPE_BF16X6; }
// the small-map schedule of the interpolator (csrc/smallmap.hip) has one emulated-fp32 form, six bf16 products on pre-split weight images;
// both fp32-grade settings of the big GEMMs take it
static inline bool afi_dtype_smallmap6(int d) { return d == AFI_DTYPE_BF16X6 || d == AFI_DTYPE_F16X3; }
namespace {
// Fork/join onto the context's side stream (created on first use, on the context's device): the weight-gradient GEMMs and bias column
// sums do not feed the data-gradient chain, so they run beside it.  Only event record / wait, so the sequence captures into a hipGraph.
// Without a context (or if the stream cannot be made) everything stays on the caller's stream.  The destructor joins, so an early
// error return never leaves side-stream work un-joined.
struct Fork {
    afi_ctx* cx; hipStream_t main, side;
    bool on;
    Fork(afi_ctx* c, hipStream_t m, bool enable) : cx(c), main(m), side(m), on(false) {
        if (enable && cx && cx->side.init()) { side = cx->side.side; on = true; after_main(); }
    }
    ~Fork() { join(); }
    void after_main() {            // work queued on `side` from here on sees everything already queued on `main`
        if (!on) return;
        hipEvent_t e = cx->side.ev();
        if (hipEventRecord(e, main) != hipSuccess || hipStreamWaitEvent(side, e, 0) != hipSuccess) { on = false; side = main; }
    }
    void join() {                  // `main` continues only after everything queued on `side`
        if (!on) return;
        hipEvent_t e = cx->side.ev();
        (void)hipEventRecord(e, side);
        (void)hipStreamWaitEvent(main, e, 0);
        on = false;
    }
};
constexpr long long kSideStreamMaxPixels = 12000;   // above this every GEMM fills the chip on its own (and overlapping kernels only perturb each other)
}  // namespace
#define AFI_CTX_CHECK(ctx) do { if (ctx) { int d_ = -1; if (hipGetDevice(&d_) != hipSuccess || d_ != ((afi_ctx*)(ctx))->device) return AFI_ERR_BAD_ARG; \
                                           ((afi_ctx*)(ctx))->amax[0].p = ((afi_ctx*)(ctx))->amax[1].p = nullptr; } } while (0)

// weight-gradient GEMM of the direct kernels under the context's options: AFI_OPT_DETERMINISTIC pins the pixel split to one block per tile
static inline bool afi_det(const afi_ctx* cx) { return afi_opt(cx, AFI_OPT_DETERMINISTIC) != 0; }
static inline int wgrad_launch(const afi_ctx* cx, AfiWgradGemm g, hipStream_t st) {
    if (afi_det(cx)) g.splitK = 1;
    return afi_launch_wgrad_gemm(g, st);
}
// per-op entry points: split-K slabs come from the context's op scratch (the whole-net calls carve theirs out of their workspace)
static inline int launch_pix_op(afi_ctx* cx, AfiPixGemm g, int b_rc, hipStream_t st) {
    if (cx && cx->op_scratch && !g.partial) { g.partial = cx->op_scratch; g.partial_floats = cx->op_scratch_floats; }
    return afi_launch_pix_gemm(g, b_rc, st);
}
static inline AfiView V(afi_view_t v) { return AfiView{v.p, v.sN, v.sH, v.sW}; }
static inline AfiView dense_view(const float* p, int H, int W, long long ld) {
    return AfiView{const_cast<float*>(p), (long long)H * W * ld, (long long)W * ld, ld};
}
static inline AfiView ch_off(AfiView v, long long c) { v.p += c; return v; }
static inline AfiView null_view() { return AfiView{nullptr, 0, 0, 0}; }
static inline long long align4(long long n) { return (n + 3) & ~3LL; }

static AfiPixGemm pix_default(int N, int H, int W) {
    AfiPixGemm g;
    memset(&g, 0, sizeof(g));
    g.N = N; g.H = H; g.W = W;
    g.ntaps = 9; g.nKphase = 1; g.a_sgn = 1; g.a_up = 1; g.o_up = 1;
    g.alpha = 1.f; g.beta = 0.f; g.r1s = 1.f; g.r2s = 1.f;
    g.a_stride = 1; g.aH = H; g.aW = W; g.oH = g.oW = 1 << 30; g.post_scale = 1.f;
    return g;
}

// forward 3x3 conv: out = act(alpha*conv(x,w) + bias + beta*out [+ residuals set by the caller])
static AfiPixGemm conv_fwd_desc(AfiView x, int N, int H, int W, int Cin, const float* w, const float* bias, int Cout, AfiView out) {
    AfiPixGemm g = pix_default(N, H, W);
    g.Ck = Cin; g.Ncols = Cout; g.CoutPhase = Cout;
    g.A = x; g.B = w; g.b_sRow = 9LL * Cin; g.b_sTap = Cin;
    g.O = out; g.bias = bias;
    return g;
}
// data gradient of a 3x3 conv with weight w[Cout][3][3][Cin]: dx = alpha*conv^T(dy) + beta*dx
static AfiPixGemm conv_dgrad_desc(AfiView dy, int N, int H, int W, int Cout, const float* w, int Cin, AfiView dx) {
    AfiPixGemm g = pix_default(N, H, W);
    g.a_sgn = -1;
    g.Ck = Cout; g.Ncols = Cin; g.CoutPhase = Cin;
    g.A = dy; g.B = w; g.b_sRow = 9LL * Cin; g.b_sTap = Cin;
    g.O = dx;
    return g;
}
static AfiWgradGemm conv_wgrad_desc(AfiView dy, AfiView x, int N, int H, int W, int Cout, int Cin, float* dw, float alpha) {
    AfiWgradGemm g;
    memset(&g, 0, sizeof(g));
    g.N = N; g.H = H; g.W = W; g.ntaps = 9;
    g.Mrows = Cout; g.Ncols = Cin;
    g.DY = dy; g.dy_up = 1; g.CoutPhase = Cout;
    g.X = x; g.DW = dw; g.dw_sRow = 9LL * Cin; g.dw_sTap = Cin;
    g.x_stride = 1; g.xH = H; g.xW = W;
    g.alpha = alpha; g.splitK = 0;
    return g;
}

// ---- Winograd F(2x2,3x3) form of a 3x3 conv (csrc/winograd.hip): weight / input transforms, ONE batched 1x1 GEMM launch over
//      the 16 transform points, output transform with the conv's epilogue.  mode 0 = forward (K = Cin, columns = Cout),
//      mode 1 = data gradient (K = Cout, columns = Cin, flipped taps).  ws: [U 16*K*Nc][V 16*Tpad*K][M 16*Tpad*Nc].
static long long wino_tpad(int N, int H, int W) { return (((long long)N * ((H + 1) / 2) * ((W + 1) / 2) + 127) / 128) * 128; }
static long long wino4_tpad(int N, int H, int W) { return (((long long)N * ((H + 3) / 4) * ((W + 3) / 4) + 127) / 128) * 128; }
// AFI_OPT_WINOGRAD_F4_FORWARD: F(4x4) tiles also for the discriminator forwards a backward follows, per block.  Their conv outputs decide LeakyReLU
// masks, so the forward's rounding shows up in the gradients as flipped masks (DESIGN.md 4 has the study): with the interpolation points of
// csrc/winograd.hip, blocks 1 and 2 on F(4x4) leave the gradients as far from an fp64 evaluation as the exact-fp32 direct kernels do (and as
// torch's own fp32 ops do); block 0 (256 input channels: the shortest sums) costs the most accuracy and buys the least time, and stays on F(2x2).
// value 1: every block; otherwise bit n + 1 selects block n (2: block 0, 4: block 1, 8: block 2; sums combine)
static bool wino_d_f4(const afi_ctx* cx, int n) { const long long v = afi_opt(cx, AFI_OPT_WINOGRAD_F4_FORWARD); return (v & 1) || ((v >> (n + 1)) & 1); }
static bool disc_local_sums(const afi_ctx* cx, int n) { const long long v = afi_opt(cx, AFI_OPT_F16_LOCAL_SUMS); return (v & 1) || ((v >> (n + 1)) & 1); }
static bool wino_f4(const afi_ctx* cx) { return afi_opt(cx, AFI_OPT_WINOGRAD_F4_BACKWARD) != 0; }
// one size for both tilings: F(2x2,3x3) = 16 transform points over 2x2 tiles, F(4x4,3x3) = 36 points over 4x4 tiles
// + the pre-split bf16 image of U the DMA GEMM stages (three 2-byte parts per element = 1.5 floats; afi_gemm_bf16.h)
// (the f16x3 image -- a 512-byte header + two 2-byte pieces per element -- fits in it: KN >= 128 x 32)
static long long wino_usplit_floats(int np, long long KN) { return align4((3 * np * KN + 1) / 2); }
// + the slots the f16x3 arithmetic's transforms raise to the largest magnitude of the tensor they read (afi_gemm_f16.h), zero-filled per call
constexpr long long kWinoAmaxFloats = 64;
// n consecutive slots (4 floats apart) at the tail of the scratch region [ws, ws + ws_floats); nullptr: the memset failed
static float* wino_amax_take(afi_ctx* cx, float* ws, long long ws_floats, int n, hipStream_t st) {
    float* pool = ws + ws_floats - kWinoAmaxFloats;
    if (!cx) return hipMemsetAsync(pool, 0, 16 * n, st) == hipSuccess ? pool : nullptr;
    afi_ctx::AmaxPool* e = cx->amax[0].p == pool ? &cx->amax[0] : (cx->amax[1].p == pool ? &cx->amax[1] : nullptr);
    if (!e || 4 * (e->next + n) > kWinoAmaxFloats) {
        if (!e) { e = cx->amax[0].p ? &cx->amax[1] : &cx->amax[0]; }
        if (hipMemsetAsync(pool, 0, sizeof(float) * kWinoAmaxFloats, st) != hipSuccess) return nullptr;
        e->p = pool; e->next = 0;
    }
    float* slot = pool + 4 * e->next;
    e->next += n;
    return slot;
}
// What a Winograd conv runs as, decided once: wino_run, wino_conv and wino_wgrad run the form, disc_plan reads it.  Kinds: a forward on F(2x2);
// a forward that may take F(4x4) (its masks decide no gradient, or AFI_OPT_WINOGRAD_F4_FORWARD names its block); a data gradient (K = Cout x nph
// phase views of a pixel-shuffled A, Nc = Cin); a weight gradient (K = Cin, Nc = Cout, nph phase views of dy).
enum WinoKind { kWinoFwd, kWinoFwdF4, kWinoDgrad, kWinoWgrad };
struct WinoForm {
    WinoKind kind; int dtype;
    bool f4; int np;           // F(4x4,3x3): 36 transform points over 4x4 tiles; else F(2x2,3x3): 16 over 2x2
    long long Tpad, T;         // tiles: padded to the GEMM's 128 rows / the map's own
    bool dma, f16;             // the LDS-DMA NT GEMM on U's pre-split image (forward / data gradient); the GEMM in f16x3
    bool presplit;             // a transform whose source maximum is known writes its planes already split (AFI_OPT_F16_PRESPLIT)
    bool keep;                 // F(4x4) and pre-split: the planes a forward writes can serve its weight gradient
};
// gradients take F(4x4,3x3) (their error decides no LeakyReLU mask), forwards only where their kind says so.  bf16 operands (2^-9) cannot carry
// the F(4x4) transforms (their 1/24 .. 8 coefficients cost two more digits: 3 % error), split-bf16 (2^-17) can; small maps have too few 4x4 tiles.
constexpr long long kWinoF4MinPixels = 8192;
static WinoForm wino_form(const afi_ctx* cx, int N, int H, int W, int K, int Nc, WinoKind kind, int nph = 1) {
    WinoForm f;
    f.kind = kind;
    f.dtype = cx ? cx->dtype : afi_default_dtype();
    f.f4 = kind != kWinoFwd && wino_f4(cx) && f.dtype != AFI_DTYPE_BF16 && (long long)N * H * W >= kWinoF4MinPixels;
    f.np = f.f4 ? 36 : 16;
    f.Tpad = f.f4 ? wino4_tpad(N, H, W) : wino_tpad(N, H, W);
    f.T = f.f4 ? (long long)N * ((H + 3) / 4) * ((W + 3) / 4) : (long long)N * ((H + 1) / 2) * ((W + 1) / 2);
    // forward / data gradient: the bf16 settings run the LDS-DMA GEMM on tile-aligned shapes (every layer of the reference nets): its B operand
    // is U split into bf16 parts in LDS-image order, made once per weight transform and cached in that form.  Weight gradient: the f16x3 TN GEMM
    // where both channel counts fill its 128-wide tiles, else the fp32 one
    const bool wgrad = kind == kWinoWgrad;
    f.dma = !wgrad && f.dtype != AFI_DTYPE_F32 && !(f.Tpad % 128) && !(Nc % 128) && !(K % 32);
    f.f16 = f.dtype == AFI_DTYPE_F16X3 && (wgrad ? !(f.Tpad % 32) && !(Nc % 128) && !(K % 128) : f.dma);
    f.presplit = afi_opt(cx, AFI_OPT_F16_PRESPLIT) != 0 && f.f16 && nph == 1;
    f.keep = f.f4 && f.presplit;
    return f;
}
// the form of a pixel-GEMM descriptor wino_eligible accepted (b_rc = 1: its data gradient)
static WinoForm wino_form(const afi_ctx* cx, const AfiPixGemm& g, int b_rc, bool fwd_f4 = false) {
    return wino_form(cx, g.N, g.H, g.W, g.Ck * g.nKphase, g.Ncols, b_rc ? kWinoDgrad : fwd_f4 ? kWinoFwdF4 : kWinoFwd, g.nKphase);
}
static long long wino_ws_floats(int N, int H, int W, int K, int Nc) {
    const long long T2 = wino_tpad(N, H, W), T4 = wino4_tpad(N, H, W);
    const long long a = align4(16LL * K * Nc) + align4(16 * T2 * K) + align4(16 * T2 * Nc) + wino_usplit_floats(16, (long long)K * Nc);
    const long long b = align4(36LL * K * Nc) + align4(36 * T4 * K) + align4(36 * T4 * Nc) + wino_usplit_floats(36, (long long)K * Nc);
    return (a > b ? a : b) + kWinoAmaxFloats;
}
// Any 3x3 / stride-1 conv DESCRIPTOR of the pixel GEMM (forward, b_rc = 0, or data gradient, b_rc = 1) run in Winograd form: the
// batched GEMM writes M, the output transform applies the descriptor's own epilogue.  Eligible: 9 taps, one K phase, no up-sampled
// gather, dense [rows][3][3][K-or-N] weights, >= 128 channels on both sides, >= 1024 pixels.
// below this many pixels a conv of the interpolator stays on the direct small-map kernels.  Scanned with tools/interp_sweep.py
// (fwd+bwd, 1024 -> 2048): 1x25x42 1.31 -> 1.04 ms, 2x25x34 1.49 -> 1.33 ms; 4096 and up lose from 3400 pixels on.
// (the workspace queries size the Winograd scratch for maps of >= 1024 pixels, so the run-time threshold cannot go below that)
static long long wino_g_minpix(const afi_ctx* cx) { const long long v = afi_opt(cx, AFI_OPT_G_WINOGRAD_MIN_PIXELS); return v < 1024 ? 1024 : v; }
static bool wino_eligible(const afi_ctx* cx, const AfiPixGemm& g, int b_rc) {
    if (!afi_opt(cx, AFI_OPT_WINOGRAD) || g.ntaps != 9 || g.gtap || g.r2_post) return false;
    // plain 3x3 conv / its data gradient, or the data gradient of the 4-phase conv-transpose (its A operand is the hi-res
    // gradient read as four phase views: each phase is one channel block of a 3x3 data gradient with 4*Cout channels)
    const bool phases = g.nKphase == 4 && g.a_up == 2 && b_rc;
    if (!phases && (g.nKphase != 1 || g.a_up != 1)) return false;
    if (g.Ck < 128 || g.Ncols < 128 || (g.Ck & 3) || (g.Ncols & 3)) return false;
    if ((long long)g.N * g.H * g.W < wino_g_minpix(cx)) return false;
    const int I = b_rc ? g.Ncols : g.Ck;                   // innermost weight dimension of w[O][3][3][I]
    return g.b_sTap == I && g.b_sRow == 9LL * I && g.a_sgn == (b_rc ? -1 : 1);
}
// Caller-owned cache of transformed weights (afi_ctx_set_wino_weight_cache): within one phase of a training step the same weights meet
// up to ten calls (five pyramid levels x real / fake), so their U = G g G^T is computed once and found again by (weight pointer,
// tiling, direction).  The caller invalidates it whenever weights change and keeps the weight memory alive while it is registered.
// returns the slot for this transform and whether it already holds it; nullptr when there is no cache or no room left
static float* wino_wcache_slot(afi_ctx* cx, const float* w, int f4, int mode, int O, int I, long long need, bool& hit) {
    hit = false;
    if (!cx || !cx->wcache.buf) return nullptr;
    WinoWeightCache& c = cx->wcache;
    for (int i = 0; i < c.n; ++i) {
        const WinoWeightCache::Entry& e = c.e[i];
        if (e.w == w && e.f4 == f4 && e.mode == mode && e.O == O && e.I == I) { hit = true; return c.buf + e.off; }
    }
    if (c.n == 128 || c.used + need > c.floats) return nullptr;
    c.e[c.n++] = WinoWeightCache::Entry{w, f4, mode, O, I, c.used};
    float* slot = c.buf + c.used;
    c.used += need;
    return slot;
}
// the cache entries a call registers for images it builds in ONE launch are committed only once that launch is issued: every exit that
// builds nothing (no room, too many jobs, a failed launch) rolls the cache back, or a later call would find the entries and multiply by
// unwritten images
struct CacheRollback {
    afi_ctx* cx; int n0; long long used0; bool keep = false;
    explicit CacheRollback(afi_ctx* c) : cx(c), n0(c ? c->wcache.n : 0), used0(c ? c->wcache.used : 0) {}
    ~CacheRollback() { if (cx && !keep) { cx->wcache.n = n0; cx->wcache.used = used0; } }
};

// ---- bf16x6 weight images of the small-map kernels (csrc/smallmap.hip: afi_pix_gemm_wk6).  A whole-net call on a small map lists the
// weights its pixel GEMMs read (forward: K-contiguous; data gradients: row-contiguous), gets every image from the context's weight cache
// when one is registered (built on first use, found again until the cache is invalidated) or builds it into the call's own workspace, all
// missing ones in ONE launch, and attaches the image to each GEMM descriptor; a descriptor without an image runs on the fp32-MFMA kernel.
constexpr long long kWk6MaxPixels = 8192;                  // workspaces reserve the image arena for calls up to this many low-res pixels
constexpr int kWk6MaxReq = 24;
// One image request: `key` names it in the cache (with b_rc: 0 forward / K-contiguous weights, 1 data gradient / row-contiguous weights); src:
// the weight it is built from.
// convT: the source is the conv-transpose weight in its torch layout [Cin][Cout][6][6] (AfiWk6ConvT; 1 the forward's image, 2 the data gradient's;
// pack_dst: the packed fp32 form written by the same launch) instead of a K- / row-contiguous matrix
struct Wk6Req { const float* key; const float* src; int Ncols, Ck, nKphase, b_rc; long long b_sRow, b_sTap; int convT; float* pack_dst; };
static inline Wk6Req wk6_req(const float* key, const float* src, int Ncols, int Ck, int nKphase, int b_rc, long long b_sRow, long long b_sTap) {
    return Wk6Req{key, src, Ncols, Ck, nKphase, b_rc, b_sRow, b_sTap, 0, nullptr};
}
static inline long long wk6_req_floats(int Ncols, int Ck, int nKphase) { return align4((afi_wk6_image_bytes(Ncols, Ck, 9, nKphase) + 3) / 4); }
struct Wk6Images {
    bool on = false;
    int n = 0;
    struct Ent { const float* key; const unsigned char* img; int nstages; } e[kWk6MaxReq];
    // the image of the weight `key`, for a problem that reads its input channels [c_lo, c_lo + g.Ck) (c_lo a multiple of 32)
    void attach(AfiPixGemm& g, const float* key, int c_lo = 0) const {
        if (!on || (c_lo & 31)) return;
        for (int i = 0; i < n; ++i)
            if (e[i].key == key) { g.Bimg = e[i].img; g.bimg_nstages = e[i].nstages; g.bimg_stage0 = (c_lo / 32) * g.ntaps; return; }
    }
};
// side (optional): work that rides in the image launch (AfiWk6Side); *side_done says whether it did -- no launch happens when every image
// came from the caller's weight cache, or when the images do not fit.  *ct_built: the conv-transpose request (Wk6Req::convT) was built here
// (and with it its packed fp32 form, when asked for), not found in the cache.
static int wk6_build(afi_ctx* cx, Wk6Images& im, const Wk6Req* reqs, int n, float* arena, long long arena_floats, hipStream_t st,
                     const AfiWk6Side* side = nullptr, bool* side_done = nullptr, bool* ct_built = nullptr) {
    im.on = false; im.n = 0;
    if (side_done) *side_done = false;
    if (ct_built) *ct_built = false;
    if (n > kWk6MaxReq) return AFI_OK;
    CacheRollback rollback(cx);
    AfiWk6ImgJob jobs[kWk6MaxReq];
    AfiWk6ConvT ct;
    bool have_ct = false;
    int nj = 0;
    long long used = 0;
    for (int i = 0; i < n; ++i) {
        const Wk6Req& r = reqs[i];
        const long long need = wk6_req_floats(r.Ncols, r.Ck, r.nKphase);
        bool hit = false;
        float* slot = wino_wcache_slot(cx, r.key, /*tags 4, 5: wk6 images*/ 4 + r.b_rc, r.nKphase, r.Ncols, r.Ck, need, hit);
        if (!slot) {
            if (!arena || used + need > arena_floats) { im.n = 0; return AFI_OK; }      // no room: the call stays on the fp32-MFMA kernels
            slot = arena + used; used += need; hit = false;
        }
        const int nst = afi_cdiv(r.Ck, 32) * 9 * r.nKphase;
        if (!hit && r.convT) {
            if (have_ct) { im.n = 0; return AFI_OK; }                                    // (one per launch)
            // forward: Ncols = 4 Cout, Ck = Cin; data gradient: Ncols = Cin, Ck = Cout
            ct = AfiWk6ConvT{r.src, (unsigned char*)slot, r.pack_dst, r.convT == 1 ? r.Ck : r.Ncols, r.convT == 1 ? r.Ncols / 4 : r.Ck, r.convT == 1 ? 0 : 1, 0};
            have_ct = true;
        } else if (!hit) {
            jobs[nj++] = AfiWk6ImgJob{r.src, r.b_sRow, r.b_sTap, r.Ncols, r.Ck, 9, r.nKphase, r.b_rc, (unsigned char*)slot};
        }
        im.e[im.n++] = Wk6Images::Ent{r.key, (const unsigned char*)slot, nst};
    }
    if (nj || have_ct) {
        AFI_TRY(afi_launch_wk6_images(jobs, nj, st, side, have_ct ? &ct : nullptr));
        if (side && side_done) *side_done = true;
        if (have_ct && ct_built) *ct_built = true;
    }
    rollback.keep = true;
    im.on = true;
    return AFI_OK;
}
// (a call lists 5 R + 4 images; the bound stays where the schedule was measured: up to three dense blocks)
static inline bool wk6_shapes_ok(int C, int G, int R) { return (C % 32) == 0 && (G % 32) == 0 && 6 * R + 4 <= kWk6MaxReq; }
// the final conv on the up-sampled map (4x the pixels) stays on the small-map kernel while the map has at most this many pixels: at config 1
// (50 x 68) the Winograd form is five launches of 9 .. 19 us (weight transform, bf16 split, input transform, GEMM, output transform)
constexpr long long kWk6HiResMaxPixels = 4096;
// arena floats of one call: every forward image / every data-gradient image of the interpolator
static long long gen_wk6_fwd_floats(int C, int G, int R, long long P) {
    if (P > kWk6MaxPixels || !wk6_shapes_ok(C, G, R)) return 0;
    const int L = C + 4 * G;
    long long f = 3 * wk6_req_floats(C, C, 1) + wk6_req_floats(4 * C, C, 1);         // head, trunk, final conv; conv-transpose
    for (int k = 1; k <= 4; ++k) f += (long long)R * wk6_req_floats(G, C + (k - 1) * G, 1);
    return f + (long long)R * wk6_req_floats(C, L, 1);
}
static long long gen_wk6_bwd_floats(int C, int G, int R, long long P) {
    if (P > kWk6MaxPixels || !wk6_shapes_ok(C, G, R)) return 0;
    const int L = C + 4 * G;
    long long f = 3 * wk6_req_floats(C, C, 1) + wk6_req_floats(C, C, 4);             // head, trunk, final conv; conv-transpose
    for (int k = 1; k <= 4; ++k) f += (long long)R * wk6_req_floats(C + (k - 1) * G, G, 1);
    return f + (long long)R * wk6_req_floats(L, C, 1);
}

// the f16x3 image of a tile-aligned conv comes straight from w (csrc/winograd.hip, afi_launch_wino_weight_images) unless bit 1 of
// AFI_OPT_F16_PRESPLIT asks for the fp32 transform + split (the A/B of the two builds: same bytes)
static inline bool wino_direct_build(const afi_ctx* cx) { return !(afi_opt(cx, AFI_OPT_F16_PRESPLIT) & 2); }
static inline bool wino_direct_image(const afi_ctx* cx, const WinoForm& f) { return f.dma && f.f16 && wino_direct_build(cx); }
// A whole-net call walks its Winograd convs at entry, in the order it runs them (add), and builds the images the context's weight cache does
// not hold yet with ONE call of the grouped builder (build: three launches) on the caller's stream; wino_run then finds hits.  The cache
// slots are taken as wino_run would take them, in the call's own order, so the cache fills exactly as it does without this; the walk
// closes at the first conv that is not on the direct path (its request then comes from wino_run, behind these); a conv the cache has no
// room for is left to wino_run as well.  Every exit without a build rolls the entries back.
// add: weight w [O][3][3][I] of a conv whose GEMM has K input and Nc output channels (data gradient: K = Cout, Nc = Cin) in the form f.
struct WinoImgBatch {
    afi_ctx* cx; CacheRollback rollback; bool open;
    AfiWinoImgJob jobs[24];
    int nj = 0;
    explicit WinoImgBatch(afi_ctx* c) : cx(c), rollback(c), open(c && c->wcache.buf && wino_direct_build(c)) {}
    void add(const float* w, int K, int Nc, const WinoForm& f) {
        if (!open) return;
        if (!wino_direct_image(cx, f) || nj == 24) { open = false; return; }
        const int b_rc = f.kind == kWinoDgrad;
        bool hit = false;
        float* slot = wino_wcache_slot(cx, w, f.f4, b_rc | (f.dtype << 4), b_rc ? K : Nc, b_rc ? Nc : K, wino_usplit_floats(f.np, (long long)K * Nc), hit);
        if (slot && !hit) jobs[nj++] = AfiWinoImgJob{w, (unsigned char*)slot, b_rc ? K : Nc, b_rc ? Nc : K, f.f4 ? 1 : 0, b_rc};
    }
    // a descriptor as GenPix will meet it (wino / n_wino: the pass's Winograd scratch)
    void add(const AfiPixGemm& g, int b_rc, long long n_wino, bool fwd_f4) {
        if (!open || g.Bimg || g.no_wcache || n_wino <= 0 || !wino_eligible(cx, g, b_rc)) return;
        add(g.B, g.Ck * g.nKphase, g.Ncols, wino_form(cx, g, b_rc, fwd_f4));
    }
    // wmax_slots: the head of the call's Winograd scratch (the U region, which the direct path leaves unused)
    int build(float* wmax_slots, hipStream_t st) {
        if (cx) AFI_TRY(afi_launch_wino_weight_images(jobs, nj, wmax_slots, st));
        rollback.keep = true;
        return AFI_OK;
    }
};

// a forward or data-gradient descriptor in the form f (wino_form of the same descriptor)
static int wino_run(afi_ctx* cx, const AfiPixGemm& g, const WinoForm& f, float* ws, long long ws_floats, float* part, long long part_floats, hipStream_t st) {
    AFI_TRY(afi_o16_refused(g));                           // (before any pass: the output transform would refuse it last)
    const int b_rc = f.kind == kWinoDgrad;
    const int nph = g.nKphase;                             // 1, or 4 phase views of a pixel-shuffled A (conv-transpose data gradient)
    const int K = g.Ck * nph, Nc = g.Ncols;
    if (ws_floats < wino_ws_floats(g.N, g.H, g.W, K, Nc)) return AFI_ERR_WORKSPACE;
    const int dtype = f.dtype, np = f.np; const long long Tpad = f.Tpad;
    const bool f4 = f.f4, dma = f.dma, f16 = f.f16;
    float* U = ws;
    float* Vb = U + align4((long long)np * K * Nc);
    float* Mb = Vb + align4(np * Tpad * K);
    float* Usp = Mb + align4(np * Tpad * Nc);              // pre-split bf16 image of U (DMA GEMM), when it is not served from the cache
    float* amax = nullptr;                                 // f16x3: the largest magnitude of A, raised by the input transform(s)
    bool have_u = false;
    if (g.no_wcache) {
    } else if (dma) {
        if (float* slot = wino_wcache_slot(cx, g.B, f4, b_rc | (dtype << 4), b_rc ? K : Nc, b_rc ? Nc : K, wino_usplit_floats(np, (long long)K * Nc), have_u)) Usp = slot;
    } else if (float* slot = wino_wcache_slot(cx, g.B, f4, b_rc, b_rc ? K : Nc, b_rc ? Nc : K, align4((long long)np * K * Nc), have_u)) U = slot;
    if (!have_u && wino_direct_image(cx, f)) {
        // one job of the grouped builder: w straight to the image; its maximum slot is the first float of the U region, which this path leaves unused
        const AfiWinoImgJob job{g.B, (unsigned char*)Usp, b_rc ? K : Nc, b_rc ? Nc : K, f4 ? 1 : 0, b_rc};
        AFI_TRY(afi_launch_wino_weight_images(&job, 1, U, st));
    } else if (!have_u) {
        // (f16x3: the weight transform raises the image header's maximum slot as it reads w, and the split takes every plane's scale from it)
        float* wmax = dma && f16 ? afi_f16_image_wmax(Usp) : nullptr;
        if (wmax) AFI_TRY(afi_f16_image_begin(Usp, st));
        AFI_TRY(f4 ? afi_launch_wino4_weight(g.B, U, b_rc ? K : Nc, b_rc ? Nc : K, b_rc, st, wmax)
                   : afi_launch_wino_weight(g.B, U, b_rc ? K : Nc, b_rc ? Nc : K, b_rc, st, wmax));
        if (dma) AFI_TRY(f16 ? afi_launch_split_f16_tiles(U, Usp, np, Nc, K, st, f4 ? 6 : 5) : afi_launch_split_bf16_tiles(U, Usp, np, Nc, K, dtype, st));
    }
    // f16x3: the largest magnitude of A.  g.a_amax given and known (its producer published it): the transform writes the planes already
    // split into fp16 pieces; given and not known: a zero-filled slot of the caller's that the transform raises (the caller keeps it, e.g. for
    // the backward pass); not given: a slot of the call's pool.
    const bool a_pre = f.presplit && g.a_amax && g.a_amax_known;
    if (f16 && !(amax = g.a_amax ? g.a_amax : wino_amax_take(cx, ws, ws_floats, 1, st))) return AFI_ERR_LAUNCH;
    const AfiF16Bound abound = afi_f16_bound(amax, f4 ? 2 : 1);
    if (g.v_keep && !(f.keep && a_pre)) return AFI_ERR_BAD_ARG;   // (never hand the weight gradient planes that were not written pre-split)
    if (g.v_keep) Vb = g.v_keep;                           // kept for the weight gradient of the same conv
    for (int ph = 0; ph < nph; ++ph) {                     // phase ph = (py, px): pixel (y, x) of its view is (2y + py, 2x + px) of A
        AfiView a = g.A;
        if (nph == 4) { a.p += (ph >> 1) * g.A.sH + (ph & 1) * g.A.sW; a.sH *= 2; a.sW *= 2; }
        // (a caller's not-yet-known slot is raised under every arithmetic: a later pass may read it)
        float* raise = g.a_amax ? (g.a_amax_known ? nullptr : g.a_amax) : (f16 ? amax : nullptr);
        AFI_TRY(f4 ? afi_launch_wino4_input(a, g.N, g.H, g.W, g.Ck, Tpad, Vb + ph * g.Ck, st, K, raise, a_pre ? &abound : nullptr)
                   : afi_launch_wino_input(a, g.N, g.H, g.W, g.Ck, Tpad, Vb + ph * g.Ck, st, K, raise, a_pre ? &abound : nullptr));
    }
    if (dma) {
        if (f16) AFI_TRY(afi_launch_gemm_nt_f16x3(Vb, Usp, Mb, np, Tpad, Nc, K, abound, st, a_pre, afi_opt(cx, AFI_OPT_F16_NT256_MIN_TILES), g.nt_local_sums != 0));
        else AFI_TRY(afi_launch_gemm_nt_bf16_dma(Vb, Usp, Mb, np, Tpad, Nc, K, dtype, st));
        return f4 ? afi_launch_wino4_output_epi(Mb, Tpad, g, st) : afi_launch_wino_output_epi(Mb, Tpad, g, st);
    }
    if (dtype == AFI_DTYPE_F32) {                          // tile-aligned shapes: the plain batched NT GEMM on the fp32 MFMA
        const int rc = afi_launch_gemm_nt(Vb, U, Mb, np, Tpad, Nc, K, st);
        if (rc == AFI_OK) return f4 ? afi_launch_wino4_output_epi(Mb, Tpad, g, st) : afi_launch_wino_output_epi(Mb, Tpad, g, st);
        if (rc != AFI_ERR_UNSUPPORTED) return rc;
    }
    AfiPixGemm q = pix_default(np, 1, (int)Tpad);
    q.ntaps = 1; q.Ck = K; q.Ncols = Nc; q.CoutPhase = Nc;
    q.A = AfiView{Vb, Tpad * K, 0, K};
    q.B = U; q.b_sRow = K; q.b_sTap = 0; q.b_sImg = (long long)K * Nc;
    q.n_fastest = 1;
    q.O = AfiView{Mb, Tpad * Nc, 0, Nc};
    q.partial = part; q.partial_floats = part_floats;
    AFI_TRY(afi_launch_pix_gemm(q, 0, st));
    return f4 ? afi_launch_wino4_output_epi(Mb, Tpad, g, st) : afi_launch_wino_output_epi(Mb, Tpad, g, st);
}

// what a whole-net call adds to a plain Winograd conv (wino_conv); every member is optional
struct WinoConvOpt {
    // forward: fp64 partial rows for the BatchNorm statistics of the output, accumulated by the output transform (afi_common.h);
    // *stats_rows: the rows written, 0 when this call did not fuse them (the caller runs the separate pass)
    double* stats = nullptr; int* stats_rows = nullptr;
    float* in_amax = nullptr; bool in_amax_known = false;   // f16x3: the slot of in's largest magnitude, and whether its producer published it
    float* v_keep = nullptr;            // forward in a keeping form (WinoForm::keep): write the input planes here, for the weight gradient
    bool local_sums = false;            // f16x3: the NT GEMM takes k-step-local sums (AFI_OPT_F16_LOCAL_SUMS)
};
// forward (kinds kWinoFwd / kWinoFwdF4: out = conv(in, w) + bias) or data gradient (kWinoDgrad: out = conv^T(in, w) * lrelu'(z)) by descriptor
static int wino_conv(afi_ctx* cx, WinoKind kind, AfiView in, int N, int H, int W, int K, const float* w, int Nc, const float* bias, AfiView out, AfiView z,
                     float* ws, long long ws_floats, float* part, long long part_floats, hipStream_t st, const WinoConvOpt& o = WinoConvOpt(),
                     bool z_relu = false) {
    if ((K & 3) || (Nc & 3)) return AFI_ERR_UNSUPPORTED;
    const bool dgrad = kind == kWinoDgrad;
    AfiPixGemm g = dgrad ? conv_dgrad_desc(in, N, H, W, K, w, Nc, out) : conv_fwd_desc(in, N, H, W, K, w, bias, Nc, out);
    g.a_amax = o.in_amax; g.a_amax_known = o.in_amax_known ? 1 : 0;
    g.v_keep = o.v_keep;
    g.nt_local_sums = o.local_sums ? 1 : 0;
    if (dgrad && z.p) { g.Z = z; g.z_lo = 0; g.z_hi = Nc; g.z_relu = z_relu ? 1 : 0; }
    const WinoForm f = wino_form(cx, g, dgrad, kind == kWinoFwdF4);
    const int rows = afi_wino_stats_rows(f.T, Nc);
    if (o.stats_rows) *o.stats_rows = 0;
    if (o.stats && o.stats_rows && !dgrad && rows > 0) { g.stats = o.stats; *o.stats_rows = rows; }
    return wino_run(cx, g, f, ws, ws_floats, part, part_floats, st);
}

// Caller-owned accumulator for the transform-domain weight gradients (afi_ctx_set_wino_wgrad_accum): dW = A'^T dU A' is linear in dU,
// so the calls of one phase that add into the same dW (five levels x real / fake) can sum their dU and transform ONCE, at
// afi_ctx_wino_wgrad_flush(), instead of zero-filling a dU and transforming it per call.
static float* wino_wgacc_slot(afi_ctx* cx, float* dw, int f4, int O, int I, float alpha, long long need, bool& fresh) {
    fresh = false;
    if (!cx || !cx->wgacc.buf) { fresh = true; return nullptr; }
    WinoWgradAccum& a = cx->wgacc;
    for (int i = 0; i < a.n; ++i) {
        const WinoWgradAccum::Entry& e = a.e[i];
        if (e.dw == dw && e.f4 == f4 && e.O == O && e.I == I) {
            if (e.alpha == alpha) return a.buf + e.off;
            fresh = true;                                  // another scale for the same target: this call goes the per-call way
            return nullptr;
        }
    }
    if (a.n == 64 || a.used + need > a.floats) { fresh = true; return nullptr; }
    a.e[a.n++] = WinoWgradAccum::Entry{dw, f4, O, I, alpha, a.used};
    float* slot = a.buf + a.used;
    a.used += need;
    fresh = true;
    return slot;
}

// weight gradient in Winograd F(3x3,2x2) form: dW[Cout][3][3][Cin] += alpha * sum_pix dy (x) x.  Same workspace layout as wino_conv
// with K = Cin, Nc = Cout:  [dU 16*Cin*Cout][V 16*Tpad*Cin][Q 16*Tpad*Cout].
// dy_phases = 4: dy is the hi-res gradient of a 4-phase conv-transpose; its phase views fill the four channel blocks of Q and
// dw is the packed weight gradient [4*CoutPhase][3][3][Cin] (Cout = 4*CoutPhase).  accumulate = false keeps the call out of the
// phase accumulator (its dw is a per-call scratch that is unpacked right away).
// what a whole-net call adds to a plain Winograd weight gradient (wino_wgrad); every member is optional
struct WinoWgradOpt {
    int dy_phases = 1; bool accumulate = true;
    // f16x3: the largest magnitudes of the two source tensors where their producers published them: both transforms then write their planes
    // already split into fp16 pieces and the GEMM stages them by DMA alone; otherwise the transforms raise two slots of the pool
    const float* dy_amax = nullptr; const float* x_amax = nullptr;
    const float* v_have = nullptr;      // the forward of this conv kept its input planes (WinoForm::keep), split with the very bound used here (x_amax)
};
static int wino_wgrad(afi_ctx* cx, AfiView dy, AfiView x, int N, int H, int W, int Cout, int Cin, float* dw, float alpha, float* ws, long long ws_floats,
                      hipStream_t st, const WinoWgradOpt& o = WinoWgradOpt()) {
    if ((Cin & 3) || (Cout & 3)) return AFI_ERR_UNSUPPORTED;
    if (ws_floats < wino_ws_floats(N, H, W, Cin, Cout)) return AFI_ERR_WORKSPACE;
    const int dy_phases = o.dy_phases;
    const WinoForm f = wino_form(cx, N, H, W, Cin, Cout, kWinoWgrad, dy_phases);     // F(3x3,4x4): 36 transform points over 4x4 blocks of dY
    const int dtype = f.dtype, np = f.np; const long long Tpad = f.Tpad;
    const bool f4 = f.f4, f16 = f.f16;
    float* dU = ws;
    float* Vb = dU + align4((long long)np * Cin * Cout);
    float* Qb = Vb + align4(np * Tpad * Cin);
    float* amax = nullptr;                                 // f16x3: [0] the largest magnitude of x, [4] of dy, raised by their transforms
    bool fresh = true, accum = false;
    if (o.accumulate)
        if (float* slot = wino_wgacc_slot(cx, dw, f4, Cout, Cin, alpha, align4((long long)np * Cin * Cout), fresh)) { dU = slot; accum = true; }
    if (fresh && hipMemsetAsync(dU, 0, sizeof(float) * np * (size_t)Cin * Cout, st) != hipSuccess) return AFI_ERR_LAUNCH;
    const bool known = f16 && o.dy_amax && o.x_amax;       // (known but not split: the in-register kernel with the known maxima; nothing is raised)
    const bool pre = f.presplit && known;
    if (f16 && !known && !(amax = wino_amax_take(cx, ws, ws_floats, 2, st))) return AFI_ERR_LAUNCH;
    const AfiF16Bound vbound = afi_f16_bound(known ? o.x_amax : amax, f4 ? 2 : 1), qbound = afi_f16_bound(known ? o.dy_amax : amax + 4, f4 ? 4 : 3);
    if (o.v_have && !(f.keep && pre)) return AFI_ERR_BAD_ARG;      // (never read planes that were not written pre-split)
    if (o.v_have) Vb = (float*)o.v_have;
    else AFI_TRY(f4 ? afi_launch_wino4_input(x, N, H, W, Cin, Tpad, Vb, st, 0, f16 && !known ? amax : nullptr, pre ? &vbound : nullptr)
                    : afi_launch_wino_input(x, N, H, W, Cin, Tpad, Vb, st, 0, f16 && !known ? amax : nullptr, pre ? &vbound : nullptr));
    const int cph = Cout / dy_phases;
    for (int ph = 0; ph < dy_phases; ++ph) {
        AfiView d = dy;
        if (dy_phases == 4) { d.p += (ph >> 1) * dy.sH + (ph & 1) * dy.sW; d.sH *= 2; d.sW *= 2; }
        AFI_TRY(f4 ? afi_launch_wino4_dy(d, N, H, W, cph, Tpad, Qb + ph * cph, st, Cout, f16 && !known ? amax + 4 : nullptr, pre ? &qbound : nullptr)
                   : afi_launch_wino_dy(d, N, H, W, cph, Tpad, Qb + ph * cph, st, Cout, f16 && !known ? amax + 4 : nullptr, pre ? &qbound : nullptr));
    }
    {   // tile-aligned shapes: the plain batched TN GEMM
        const bool det = afi_det(cx);
        const int rc = dtype == AFI_DTYPE_F32 || (dtype == AFI_DTYPE_F16X3 && !f16) ? afi_launch_gemm_tn(Qb, Vb, dU, np, Tpad, Cout, Cin, st, det)
                     : f16 ? afi_launch_gemm_tn_f16x3(Qb, Vb, dU, np, Tpad, Cout, Cin, qbound, vbound, st, pre, det)
                           : afi_launch_gemm_tn_bf16(Qb, Vb, dU, np, Tpad, Cout, Cin, dtype, st, det);
        if (rc == AFI_OK) {
            if (accum) return AFI_OK;                      // transformed at afi_wino_wgrad_flush()
            return f4 ? afi_launch_wino4_dw(dU, dw, Cout, Cin, alpha, st) : afi_launch_wino_dw(dU, dw, Cout, Cin, alpha, st);
        }
        if (rc != AFI_ERR_UNSUPPORTED) return rc;
    }
    AfiWgradGemm g;
    memset(&g, 0, sizeof(g));
    g.N = 1; g.H = 1; g.W = (int)Tpad; g.ntaps = np;
    g.Mrows = Cout; g.Ncols = Cin;
    g.DY = AfiView{Qb, 0, 0, Cout}; g.dy_up = 1; g.CoutPhase = Cout; g.dy_sTap = Tpad * Cout;
    g.X = AfiView{Vb, 0, 0, Cin}; g.x_stride = 1; g.xH = 1; g.xW = (int)Tpad; g.x_sTap = Tpad * Cin;
    g.DW = dU; g.dw_sRow = Cin; g.dw_sTap = (long long)Cout * Cin;
    g.alpha = 1.f; g.splitK = 0;
    AFI_TRY(wgrad_launch(cx, g, st));
    if (accum) return AFI_OK;
    return f4 ? afi_launch_wino4_dw(dU, dw, Cout, Cin, alpha, st) : afi_launch_wino_dw(dU, dw, Cout, Cin, alpha, st);
}

static long long disc_wino_floats(const int F[4], int N, int H, int W) {
    if ((long long)N * H * W < 1024) return 0;
    long long m = 0;
    for (int n = 0; n < 3; ++n) { const long long v = wino_ws_floats(N, H, W, F[n], F[n + 1]); if (v > m) m = v; }
    return m;
}

extern "C" {

int afi_debug_wk6_convT_images(const float* W, int Cin, int Cout, int mode, void* direct, float* pack_ride, void* via_pack, float* pack_ref,
                               long long* bytes, void* stream) {
    if (Cin <= 0 || Cout <= 0 || (Cin & 31) || (Cout & 31) || (mode != 0 && mode != 1) || !bytes) return AFI_ERR_BAD_ARG;
    *bytes = mode == 0 ? afi_wk6_image_bytes(4 * Cout, Cin, 9, 1) : afi_wk6_image_bytes(Cin, Cout, 9, 4);
    if (!W && !direct && !via_pack) return AFI_OK;
    if (!W || !direct || !pack_ride || !via_pack || !pack_ref) return AFI_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    const AfiWk6ConvT ct{W, (unsigned char*)direct, pack_ride, Cin, Cout, mode, 0};
    AFI_TRY(afi_launch_wk6_images(nullptr, 0, st, nullptr, &ct));
    AFI_TRY(afi_launch_convT_pack(W, pack_ref, Cin, Cout, st));
    const AfiWk6ImgJob job = mode == 0 ? AfiWk6ImgJob{pack_ref, 9LL * Cin, Cin, 4 * Cout, Cin, 9, 1, 0, (unsigned char*)via_pack}
                                       : AfiWk6ImgJob{pack_ref, 9LL * Cin, Cin, Cin, Cout, 9, 4, 1, (unsigned char*)via_pack};
    return afi_launch_wk6_images(&job, 1, st, nullptr, nullptr);
}
int afi_abi_version(void) { return 9; }
// digest of the sources this binary was compiled from (__graft_entry__.build() writes csrc/afi_build_id.h in front of the compile:
// sha256 over every *.hip / *.h of csrc/ and include/afigan_hip.h, the generated header excluded).  The Python binding recomputes it from the
// tree it sits in and refuses a library built from other sources; smoke() prints it.
#if __has_include("afi_build_id.h")
#include "afi_build_id.h"
#else
#define AFI_BUILD_ID "unknown"
#endif
const char* afi_build_id(void) { return AFI_BUILD_ID; }

const char* afi_status_string(int s) {
    switch (s) {
        case AFI_OK: return "ok";
        case AFI_ERR_BAD_ARG: return "bad argument";
        case AFI_ERR_UNSUPPORTED: return "unsupported shape (channel counts must be multiples of 4)";
        case AFI_ERR_LAUNCH: return "HIP kernel launch failed";
        case AFI_ERR_WORKSPACE: return "workspace too small";
        default: return "unknown status";
    }
}

// ------------------------------------------------------------------------------------------------ context
int afi_ctx_create(afi_ctx_t** out) {
    if (!out) return AFI_ERR_BAD_ARG;
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) return AFI_ERR_LAUNCH;
    afi_ctx* cx = new (std::nothrow) afi_ctx();
    if (!cx) return AFI_ERR_WORKSPACE;
    cx->device = dev;
    *out = cx;
    return AFI_OK;
}
int afi_ctx_destroy(afi_ctx_t* ctx) {
    if (!ctx) return AFI_OK;
    afi_ctx* cx = ctx;
    if (cx->wgacc.n != 0) return AFI_ERR_BAD_ARG;          // pending weight-gradient sums: flush or discard first
    cx->side.destroy();
    delete cx;
    return AFI_OK;
}
int afi_ctx_set_compute_dtype(afi_ctx_t* ctx, int dtype) {
    if (!ctx || !afi_dtype_ok(dtype)) return AFI_ERR_BAD_ARG;
    if (ctx->wgacc.n) return AFI_ERR_BAD_ARG;             // pending transform-domain sums belong to the tiling of the old setting
    ctx->dtype = dtype;
    return AFI_OK;
}
int afi_ctx_get_compute_dtype(const afi_ctx_t* ctx) { return ctx ? ctx->dtype : afi_default_dtype(); }
int afi_ctx_set_option(afi_ctx_t* ctx, int option, long long value) {
    if (!ctx || option < 0 || option >= AFI_OPT_COUNT || value < 0) return AFI_ERR_BAD_ARG;
    if (ctx->wgacc.n) return AFI_ERR_BAD_ARG;             // pending transform-domain sums belong to the tiling of the old setting
    ctx->opt.v[option] = value;
    return AFI_OK;
}
long long afi_ctx_get_option(const afi_ctx_t* ctx, int option) {
    if (option < 0 || option >= AFI_OPT_COUNT) return -1;
    return afi_opt(ctx, option);
}
long long afi_gemm_nt_scratch_bytes(int planes, int N, int K, int dtype) {
    if (planes <= 0 || N <= 0 || K <= 0) return -1;
    if (dtype == AFI_DTYPE_F32) return 0;
    if (!afi_dtype_ok(dtype)) return -1;
    if (dtype == AFI_DTYPE_F16X3) return afi_f16_image_bytes(planes, N, K) + 256;      // + the per-plane maxima of A
    return (long long)planes * N * K * 2 * (dtype == AFI_DTYPE_BF16X6 ? 3 : (dtype == AFI_DTYPE_BF16X3 ? 2 : 1));
}
int afi_gemm_nt(const float* A, const float* B, float* C, int planes, long long rows_per_plane, int N, int K, int dtype, void* scratch, long long scratch_bytes,
                void* stream) {
    if (!A || !B || !C) return AFI_ERR_BAD_ARG;
    if (dtype == AFI_DTYPE_F32) return afi_launch_gemm_nt(A, B, C, planes, rows_per_plane, N, K, (hipStream_t)stream);
    if (!afi_dtype_ok(dtype)) return AFI_ERR_BAD_ARG;
    if (planes <= 0 || rows_per_plane <= 0 || N <= 0 || K <= 0) return AFI_ERR_BAD_ARG;
    if ((rows_per_plane % 128) || (N % 128) || (K % 32)) return AFI_ERR_UNSUPPORTED;
    if (!scratch || scratch_bytes < afi_gemm_nt_scratch_bytes(planes, N, K, dtype)) return AFI_ERR_WORKSPACE;
    if (dtype == AFI_DTYPE_F16X3) {
        // stand-alone: the exact per-plane maxima of both operands, by a pass over each (inside a convolution the transforms that write
        // the planes provide a bound as a by-product and no pass exists)
        if (planes > 36) return AFI_ERR_UNSUPPORTED;
        hipStream_t st = (hipStream_t)stream;
        float* amax = (float*)((unsigned char*)scratch + afi_f16_image_bytes(planes, N, K));
        if (hipMemsetAsync(amax, 0, 256, st) != hipSuccess) return AFI_ERR_LAUNCH;
        AFI_TRY(afi_launch_absmax_planes(A, rows_per_plane * K, planes, amax, st));
        AFI_TRY(afi_launch_split_f16_tiles(B, scratch, planes, N, K, st));
        return afi_launch_gemm_nt_f16x3(A, scratch, C, planes, rows_per_plane, N, K, afi_f16_bound(amax, 0), st);
    }
    AFI_TRY(afi_launch_split_bf16_tiles(B, scratch, planes, N, K, dtype, (hipStream_t)stream));
    return afi_launch_gemm_nt_bf16_dma(A, scratch, C, planes, rows_per_plane, N, K, dtype, (hipStream_t)stream);
}
long long afi_gemm_tn_scratch_bytes(int planes, int dtype) {
    if (planes <= 0 || !afi_dtype_ok(dtype)) return -1;
    return dtype == AFI_DTYPE_F16X3 ? 512 : 0;
}
int afi_gemm_tn(const float* Q, const float* V, float* dU, int planes, long long rows_per_plane, int M, int N, int dtype, void* scratch, long long scratch_bytes,
                void* stream) {
    if (!Q || !V || !dU) return AFI_ERR_BAD_ARG;
    if (dtype == AFI_DTYPE_F32) return afi_launch_gemm_tn(Q, V, dU, planes, rows_per_plane, M, N, (hipStream_t)stream);
    if (!afi_dtype_ok(dtype)) return AFI_ERR_BAD_ARG;
    if (dtype == AFI_DTYPE_F16X3) {
        if (planes <= 0 || rows_per_plane <= 0 || M <= 0 || N <= 0) return AFI_ERR_BAD_ARG;
        if (planes > 36 || (rows_per_plane % 32) || (M % 128) || (N % 128)) return AFI_ERR_UNSUPPORTED;
        if (!scratch || scratch_bytes < 512) return AFI_ERR_WORKSPACE;
        hipStream_t st = (hipStream_t)stream;
        float* amax = (float*)scratch;
        if (hipMemsetAsync(amax, 0, 512, st) != hipSuccess) return AFI_ERR_LAUNCH;
        AFI_TRY(afi_launch_absmax_planes(Q, rows_per_plane * M, planes, amax, st));
        AFI_TRY(afi_launch_absmax_planes(V, rows_per_plane * N, planes, amax + 64, st));
        return afi_launch_gemm_tn_f16x3(Q, V, dU, planes, rows_per_plane, M, N, afi_f16_bound(amax, 0), afi_f16_bound(amax + 64, 0), st);
    }
    return afi_launch_gemm_tn_bf16(Q, V, dU, planes, rows_per_plane, M, N, dtype, (hipStream_t)stream);
}
int afi_ctx_set_op_scratch(afi_ctx_t* ctx, float* p, long long floats) {
    if (!ctx || floats < 0 || (floats > 0 && !p)) return AFI_ERR_BAD_ARG;
    ctx->op_scratch = floats > 0 ? p : nullptr;
    ctx->op_scratch_floats = floats > 0 ? floats : 0;
    return AFI_OK;
}
int afi_ctx_set_wino_weight_cache(afi_ctx_t* ctx, float* buf, long long floats) {
    if (!ctx || floats < 0 || (floats > 0 && !buf)) return AFI_ERR_BAD_ARG;
    ctx->wcache.buf = floats > 0 ? buf : nullptr;
    ctx->wcache.floats = floats; ctx->wcache.used = 0; ctx->wcache.n = 0;
    return AFI_OK;
}
int afi_ctx_wino_weight_cache_invalidate(afi_ctx_t* ctx) {
    if (!ctx) return AFI_ERR_BAD_ARG;
    ctx->wcache.used = 0; ctx->wcache.n = 0;
    return AFI_OK;
}
int afi_ctx_set_wino_wgrad_accum(afi_ctx_t* ctx, float* buf, long long floats) {
    if (!ctx || floats < 0 || (floats > 0 && !buf) || ctx->wgacc.n != 0) return AFI_ERR_BAD_ARG;      // pending sums must be flushed first
    ctx->wgacc.buf = floats > 0 ? buf : nullptr;
    ctx->wgacc.floats = floats; ctx->wgacc.used = 0;
    return AFI_OK;
}
int afi_ctx_wino_wgrad_flush(afi_ctx_t* ctx, void* stream) {
    if (!ctx) return AFI_ERR_BAD_ARG;
    AFI_CTX_CHECK(ctx);
    hipStream_t st = (hipStream_t)stream;
    WinoWgradAccum& a = ctx->wgacc;
    int rc = AFI_OK;
    for (int i = 0; i < a.n && rc == AFI_OK; ++i) {
        const WinoWgradAccum::Entry& e = a.e[i];
        rc = e.f4 ? afi_launch_wino4_dw(a.buf + e.off, e.dw, e.O, e.I, e.alpha, st) : afi_launch_wino_dw(a.buf + e.off, e.dw, e.O, e.I, e.alpha, st);
    }
    a.n = 0; a.used = 0;
    return rc;
}
int afi_ctx_wino_wgrad_discard(afi_ctx_t* ctx) {           // error path: drop the pending sums instead of adding partial ones into dW
    if (!ctx) return AFI_ERR_BAD_ARG;
    ctx->wgacc.n = 0; ctx->wgacc.used = 0;
    return AFI_OK;
}

// ------------------------------------------------------------------------------------------------ per-op
int afi_conv3x3_fwd(afi_ctx_t* ctx, afi_view_t x, int N, int H, int W, int Cin, const float* w, const float* bias, int Cout, afi_view_t out, float alpha,
                    float beta, int lrelu, void* stream) {
    afi_ctx* cx = ctx; (void)cx;
    AFI_CTX_CHECK(ctx);
    if ((Cin & 3) || (Cout & 3)) return AFI_ERR_UNSUPPORTED;     // float4 granularity of loads and of the epilogue stores
    AfiPixGemm g = conv_fwd_desc(V(x), N, H, W, Cin, w, bias, Cout, V(out));
    g.alpha = alpha; g.beta = beta; g.lrelu = lrelu;
    return launch_pix_op(cx, g, 0, (hipStream_t)stream);
}
int afi_conv3x3_fwd_out16(afi_ctx_t* ctx, afi_view_t x, int N, int H, int W, int Cin, const float* w, const float* bias, int Cout, afi_view_t out,
                          int out_dtype, float alpha, float beta, int lrelu, void* stream) {
    afi_ctx* cx = ctx; (void)cx;
    AFI_CTX_CHECK(ctx);
    if (out_dtype != AFI_STORE_BF16 && out_dtype != AFI_STORE_F16) return AFI_ERR_BAD_ARG;
    if ((Cin & 3) || (Cout & 3)) return AFI_ERR_UNSUPPORTED;
    AfiPixGemm g = conv_fwd_desc(V(x), N, H, W, Cin, w, bias, Cout, V(out));
    g.alpha = alpha; g.beta = beta; g.lrelu = lrelu; g.o_dtype = out_dtype;
    return launch_pix_op(cx, g, 0, (hipStream_t)stream);
}
int afi_conv3x3_dgrad(afi_ctx_t* ctx, afi_view_t dy, int N, int H, int W, int Cout, const float* w, int Cin, afi_view_t dx, float alpha, float beta,
                      afi_view_t z, void* stream) {
    afi_ctx* cx = ctx; (void)cx;
    AFI_CTX_CHECK(ctx);
    if ((Cin & 3) || (Cout & 3)) return AFI_ERR_UNSUPPORTED;
    AfiPixGemm g = conv_dgrad_desc(V(dy), N, H, W, Cout, w, Cin, V(dx));
    g.alpha = alpha; g.beta = beta;
    if (z.p) { g.Z = V(z); g.z_lo = 0; g.z_hi = Cin; }
    return launch_pix_op(cx, g, 1, (hipStream_t)stream);
}
int afi_conv3x3_wgrad(afi_ctx_t* ctx, afi_view_t dy, afi_view_t x, int N, int H, int W, int Cout, int Cin, float* dw, float alpha, void* stream) {
    afi_ctx* cx = ctx; (void)cx;
    AFI_CTX_CHECK(ctx);
    if ((Cin & 3) || (Cout & 3)) return AFI_ERR_UNSUPPORTED;
    return wgrad_launch(cx, conv_wgrad_desc(V(dy), V(x), N, H, W, Cout, Cin, dw, alpha), (hipStream_t)stream);
}

long long afi_conv3x3_wino_ws_floats(int N, int H, int W, int Cin, int Cout) { return wino_ws_floats(N, H, W, Cin, Cout); }
int afi_conv3x3_wino_fwd(afi_ctx_t* ctx, afi_view_t x, int N, int H, int W, int Cin, const float* w, const float* bias, int Cout, afi_view_t out, float* ws,
                         long long ws_floats, void* stream) {
    afi_ctx* cx = ctx; (void)cx;
    AFI_CTX_CHECK(ctx);
    if (N <= 0 || H <= 0 || W <= 0 || !ws) return AFI_ERR_BAD_ARG;
    return wino_conv(cx, kWinoFwd, V(x), N, H, W, Cin, w, Cout, bias, V(out), null_view(), ws, ws_floats, nullptr, 0, (hipStream_t)stream);
}
int afi_conv3x3_wino_fwd_out16(afi_ctx_t* ctx, afi_view_t x, int N, int H, int W, int Cin, const float* w, const float* bias, int Cout, afi_view_t out,
                               int out_dtype, float* ws, long long ws_floats, void* stream) {
    afi_ctx* cx = ctx; (void)cx;
    AFI_CTX_CHECK(ctx);
    if (out_dtype != AFI_STORE_BF16 && out_dtype != AFI_STORE_F16) return AFI_ERR_BAD_ARG;
    if (N <= 0 || H <= 0 || W <= 0 || !ws) return AFI_ERR_BAD_ARG;
    if ((Cin & 3) || (Cout & 3)) return AFI_ERR_UNSUPPORTED;
    AfiPixGemm g = conv_fwd_desc(V(x), N, H, W, Cin, w, bias, Cout, V(out));
    g.o_dtype = out_dtype;
    return wino_run(cx, g, wino_form(cx, g, 0), ws, ws_floats, nullptr, 0, (hipStream_t)stream);
}
int afi_conv3x3_wino_infer(afi_ctx_t* ctx, afi_view_t x, int N, int H, int W, int Cin, const float* w, const float* bias, int Cout, afi_view_t out, int act,
                           float* ws, long long ws_floats, void* stream) {
    afi_ctx* cx = ctx; (void)cx;
    AFI_CTX_CHECK(ctx);
    if (N <= 0 || H <= 0 || W <= 0 || !ws || act < 0 || act > 2) return AFI_ERR_BAD_ARG;
    if ((Cin & 3) || (Cout & 3)) return AFI_ERR_UNSUPPORTED;
    AfiPixGemm g = conv_fwd_desc(V(x), N, H, W, Cin, w, bias, Cout, V(out));
    g.lrelu = act;
    return wino_run(cx, g, wino_form(cx, g, 0, /*fwd_f4=*/true), ws, ws_floats, nullptr, 0, (hipStream_t)stream);
}
int afi_conv3x3_wino_dgrad(afi_ctx_t* ctx, afi_view_t dy, int N, int H, int W, int Cout, const float* w, int Cin, afi_view_t dx, afi_view_t z, float* ws,
                           long long ws_floats, void* stream) {
    afi_ctx* cx = ctx; (void)cx;
    AFI_CTX_CHECK(ctx);
    if (N <= 0 || H <= 0 || W <= 0 || !ws) return AFI_ERR_BAD_ARG;
    return wino_conv(cx, kWinoDgrad, V(dy), N, H, W, Cout, w, Cin, nullptr, V(dx), z.p ? V(z) : null_view(), ws, ws_floats, nullptr, 0, (hipStream_t)stream);
}

int afi_conv3x3_wino_wgrad(afi_ctx_t* ctx, afi_view_t dy, afi_view_t x, int N, int H, int W, int Cout, int Cin, float* dw, float alpha, float* ws,
                           long long ws_floats, void* stream) {
    afi_ctx* cx = ctx; (void)cx;
    AFI_CTX_CHECK(ctx);
    if (N <= 0 || H <= 0 || W <= 0 || !ws || !dw) return AFI_ERR_BAD_ARG;
    return wino_wgrad(cx, V(dy), V(x), N, H, W, Cout, Cin, dw, alpha, ws, ws_floats, (hipStream_t)stream);
}

int afi_conv1x1_fwd(afi_ctx_t* ctx, afi_view_t x, int N, int H, int W, int Cin, const float* w, const float* bias, int Cout, afi_view_t out, float alpha,
                    float beta, afi_view_t r1, float r1_scale, int lrelu, void* stream) {
    afi_ctx* cx = ctx; (void)cx;
    AFI_CTX_CHECK(ctx);
    if ((Cin & 3) || (Cout & 3)) return AFI_ERR_UNSUPPORTED;
    AfiPixGemm g = pix_default(N, H, W);
    g.ntaps = 1; g.Ck = Cin; g.Ncols = Cout; g.CoutPhase = Cout;
    g.A = V(x); g.B = w; g.b_sRow = Cin; g.b_sTap = 0;
    g.O = V(out); g.bias = bias; g.alpha = alpha; g.beta = beta; g.lrelu = lrelu;
    if (r1.p) { g.R1 = V(r1); g.r1s = r1_scale; g.r1_lo = 0; g.r1_hi = Cout; }
    return launch_pix_op(cx, g, 0, (hipStream_t)stream);
}
int afi_conv1x1_dgrad(afi_ctx_t* ctx, afi_view_t dy, int N, int H, int W, int Cout, const float* w, int Cin, afi_view_t dx, float alpha, float beta,
                      void* stream) {
    afi_ctx* cx = ctx; (void)cx;
    AFI_CTX_CHECK(ctx);
    if ((Cin & 3) || (Cout & 3)) return AFI_ERR_UNSUPPORTED;
    AfiPixGemm g = pix_default(N, H, W);
    g.ntaps = 1; g.a_sgn = -1; g.Ck = Cout; g.Ncols = Cin; g.CoutPhase = Cin;
    g.A = V(dy); g.B = w; g.b_sRow = Cin; g.b_sTap = 0;
    g.O = V(dx); g.alpha = alpha; g.beta = beta;
    return launch_pix_op(cx, g, 1, (hipStream_t)stream);
}
// ---- data gradients with the activation's mask by kind (z_act 1: LeakyReLU(0.2), 2: ReLU): the backward of a conv whose input is act(z).
// The mask is the epilogue's last factor, so with beta / add it covers the join as well: dx = (alpha W^T dy + beta dx + add_scale add) * act'(z).
// beta != 0 reads dx in the epilogue only, by the thread that stores the element -- in the whole-tile kernels and in the second pass of every
// split-K / stream-K form alike (their first pass leaves raw partial sums in slabs) --, so dx may be updated in place.
static int z_act_set(AfiPixGemm& g, afi_view_t z, int z_act, int Cin) {
    if (!z.p) return AFI_OK;
    if (z_act != 1 && z_act != 2) return AFI_ERR_BAD_ARG;
    g.Z = V(z); g.z_lo = 0; g.z_hi = Cin; g.z_relu = z_act == 2;
    return AFI_OK;
}
int afi_conv1x1_dgrad_act(afi_ctx_t* ctx, afi_view_t dy, int N, int H, int W, int Cout, const float* w, int Cin, afi_view_t dx, float alpha, float beta,
                          afi_view_t add, float add_scale, afi_view_t z, int z_act, void* stream) {
    afi_ctx* cx = ctx; (void)cx;
    AFI_CTX_CHECK(ctx);
    if ((Cin & 3) || (Cout & 3)) return AFI_ERR_UNSUPPORTED;
    AfiPixGemm g = pix_default(N, H, W);
    g.ntaps = 1; g.a_sgn = -1; g.Ck = Cout; g.Ncols = Cin; g.CoutPhase = Cin;
    g.A = V(dy); g.B = w; g.b_sRow = Cin; g.b_sTap = 0;
    g.O = V(dx); g.alpha = alpha; g.beta = beta;
    if (add.p) { g.R1 = V(add); g.r1s = add_scale; g.r1_lo = 0; g.r1_hi = Cin; }
    AFI_TRY(z_act_set(g, z, z_act, Cin));
    return launch_pix_op(cx, g, 1, (hipStream_t)stream);
}
int afi_conv3x3_dgrad_act(afi_ctx_t* ctx, afi_view_t dy, int N, int H, int W, int Cout, const float* w, int Cin, afi_view_t dx, float alpha, float beta,
                          afi_view_t z, int z_act, void* stream) {
    afi_ctx* cx = ctx; (void)cx;
    AFI_CTX_CHECK(ctx);
    if ((Cin & 3) || (Cout & 3)) return AFI_ERR_UNSUPPORTED;
    AfiPixGemm g = conv_dgrad_desc(V(dy), N, H, W, Cout, w, Cin, V(dx));
    g.alpha = alpha; g.beta = beta;
    AFI_TRY(z_act_set(g, z, z_act, Cin));
    return launch_pix_op(cx, g, 1, (hipStream_t)stream);
}
int afi_conv3x3_wino_dgrad_act(afi_ctx_t* ctx, afi_view_t dy, int N, int H, int W, int Cout, const float* w, int Cin, afi_view_t dx, afi_view_t z, int z_act,
                               float* ws, long long ws_floats, void* stream) {
    afi_ctx* cx = ctx; (void)cx;
    AFI_CTX_CHECK(ctx);
    if (N <= 0 || H <= 0 || W <= 0 || !ws) return AFI_ERR_BAD_ARG;
    if (z.p && z_act != 1 && z_act != 2) return AFI_ERR_BAD_ARG;
    return wino_conv(cx, kWinoDgrad, V(dy), N, H, W, Cout, w, Cin, nullptr, V(dx), z.p ? V(z) : null_view(), ws, ws_floats, nullptr, 0, (hipStream_t)stream,
                     WinoConvOpt(), z.p && z_act == 2);
}
int afi_conv1x1_dgrad_out16(afi_ctx_t* ctx, afi_view_t dy, int N, int H, int W, int Cout, const float* w, int Cin, afi_view_t dx, int dx_dtype, float alpha,
                            float beta, void* stream) {
    afi_ctx* cx = ctx; (void)cx;
    AFI_CTX_CHECK(ctx);
    if (dx_dtype != AFI_STORE_BF16 && dx_dtype != AFI_STORE_F16) return AFI_ERR_BAD_ARG;
    if ((Cin & 3) || (Cout & 3)) return AFI_ERR_UNSUPPORTED;
    AfiPixGemm g = pix_default(N, H, W);
    g.ntaps = 1; g.a_sgn = -1; g.Ck = Cout; g.Ncols = Cin; g.CoutPhase = Cin;
    g.A = V(dy); g.B = w; g.b_sRow = Cin; g.b_sTap = 0;
    g.O = V(dx); g.alpha = alpha; g.beta = beta; g.o_dtype = dx_dtype;
    return launch_pix_op(cx, g, 1, (hipStream_t)stream);
}
int afi_conv1x1_wgrad(afi_ctx_t* ctx, afi_view_t dy, afi_view_t x, int N, int H, int W, int Cout, int Cin, float* dw, float alpha, void* stream) {
    afi_ctx* cx = ctx; (void)cx;
    AFI_CTX_CHECK(ctx);
    if ((Cin & 3) || (Cout & 3)) return AFI_ERR_UNSUPPORTED;
    AfiWgradGemm g = conv_wgrad_desc(V(dy), V(x), N, H, W, Cout, Cin, dw, alpha);
    g.ntaps = 1; g.dw_sRow = Cin; g.dw_sTap = 0;
    return wgrad_launch(cx, g, (hipStream_t)stream);
}

// ---- Conv2d(k=3, stride=2, padding=1): the PAFPN bottom-up downsample (pafpn_sr.py:105-117,178-183) ----
// forward: rows are the Ho x Wo output pixels (Ho = ceil(Hi/2)), tap t reads x[2y + t/3 - 1][2x + t%3 - 1]
int afi_conv3x3s2_fwd(afi_ctx_t* ctx, afi_view_t x, int N, int Hi, int Wi, int Cin, const float* w, const float* bias, int Cout, afi_view_t out, int act,
                      afi_view_t act_out, float post_scale, afi_view_t r, float r_scale, void* stream) {
    afi_ctx* cx = ctx; (void)cx;
    AFI_CTX_CHECK(ctx);
    if ((Cin & 3) || (Cout & 3)) return AFI_ERR_UNSUPPORTED;
    if (Hi < 1 || Wi < 1) return AFI_ERR_BAD_ARG;
    const int Ho = (Hi + 1) / 2, Wo = (Wi + 1) / 2;
    AfiPixGemm g = conv_fwd_desc(V(x), N, Ho, Wo, Cin, w, bias, Cout, V(out));
    g.gtap = 1; g.a_stride = 2; g.aH = Hi; g.aW = Wi;
    for (int t = 0; t < 9; ++t) { g.tap_dy[t] = (signed char)(t / 3 - 1); g.tap_dx[t] = (signed char)(t % 3 - 1); g.tap_w[t] = (signed char)t; }
    g.lrelu = act; g.r2_post = 1; g.post_scale = post_scale;
    if (act_out.p) g.O2 = V(act_out);
    if (r.p) { g.R2 = V(r); g.r2s = r_scale; g.r2_lo = 0; g.r2_hi = Cout; }
    return launch_pix_op(cx, g, 0, (hipStream_t)stream);
}
// data gradient: input pixel (2m + py, 2n + px) only sees the taps of matching parity -- ky = 1 for py = 0 (dy row m), ky = 0 / 2
// for py = 1 (dy rows m+1 / m) -- so dx is four GEMMs over the Ho x Wo grid with 1, 2, 2 and 4 taps (9 in total: no wasted
// MFMA work, unlike a stride-1 dgrad over a zero-stuffed dy which would do 4x), each storing its parity phase of dx.
int afi_conv3x3s2_dgrad(afi_ctx_t* ctx, afi_view_t dy, int N, int Hi, int Wi, int Cout, const float* w, int Cin, afi_view_t dx, float alpha, float beta,
                        void* stream) {
    afi_ctx* cx = ctx; (void)cx;
    AFI_CTX_CHECK(ctx);
    if ((Cin & 3) || (Cout & 3)) return AFI_ERR_UNSUPPORTED;
    if (Hi < 1 || Wi < 1) return AFI_ERR_BAD_ARG;
    const int Ho = (Hi + 1) / 2, Wo = (Wi + 1) / 2;
    for (int ph = 0; ph < 4; ++ph) {
        const int py = ph >> 1, px = ph & 1;
        if (Hi - py <= 0 || Wi - px <= 0) continue;
        AfiPixGemm g = pix_default(N, Ho, Wo);
        g.Ck = Cout; g.Ncols = Cin; g.CoutPhase = Cin;
        g.A = V(dy); g.B = w; g.b_sRow = 9LL * Cin; g.b_sTap = Cin;
        g.gtap = 1;
        int nt = 0;
        for (int iy = 0; iy < (py ? 2 : 1); ++iy)
            for (int ix = 0; ix < (px ? 2 : 1); ++ix) {
                const int ky = py ? (iy ? 2 : 0) : 1, kx = px ? (ix ? 2 : 0) : 1;
                g.tap_dy[nt] = (signed char)(py && !iy ? 1 : 0);
                g.tap_dx[nt] = (signed char)(px && !ix ? 1 : 0);
                g.tap_w[nt] = (signed char)(ky * 3 + kx);
                ++nt;
            }
        g.ntaps = nt;
        AfiView o = V(dx);
        o.p += py * o.sH + px * o.sW;
        g.O = o; g.o_up = 2; g.oH = Hi - py; g.oW = Wi - px;
        g.alpha = alpha; g.beta = beta;
        const int rc = launch_pix_op(cx, g, 1, (hipStream_t)stream);
        if (rc != AFI_OK) return rc;
    }
    return AFI_OK;
}
int afi_conv3x3s2_wgrad(afi_ctx_t* ctx, afi_view_t dy, afi_view_t x, int N, int Hi, int Wi, int Cout, int Cin, float* dw, float alpha, void* stream) {
    afi_ctx* cx = ctx; (void)cx;
    AFI_CTX_CHECK(ctx);
    if ((Cin & 3) || (Cout & 3)) return AFI_ERR_UNSUPPORTED;
    if (Hi < 1 || Wi < 1) return AFI_ERR_BAD_ARG;
    AfiWgradGemm g = conv_wgrad_desc(V(dy), V(x), N, (Hi + 1) / 2, (Wi + 1) / 2, Cout, Cin, dw, alpha);
    g.x_stride = 2; g.xH = Hi; g.xW = Wi;
    return wgrad_launch(cx, g, (hipStream_t)stream);
}
int afi_relu_bwd(const float* g, const float* act, float* out, long long n, float scale, void* stream) {
    return afi_launch_relu_bwd(g, act, out, n, scale, (hipStream_t)stream);
}

// ---- BiFPN inference pieces (bifpn_sr.py; forward only: the reference ships BiFPN in an inference config only) ----
int afi_dwconv3x3_fwd(afi_view_t x, int N, int H, int W, int C, const float* w9c, float* out, void* stream) {
    return afi_launch_dwconv3x3(V(x), N, H, W, C, w9c, out, (hipStream_t)stream);
}
int afi_maxpool3s2_same_fwd(afi_view_t x, int N, int H, int W, int C, float* out, void* stream) {
    return afi_launch_maxpool3s2_same(V(x), N, H, W, C, out, (hipStream_t)stream);
}
int afi_fuse_swish_fwd(const float* a, const float* b, const float* c_or_null, const float* w_dev, float* out, long long n, void* stream) {
    return afi_launch_fuse_swish(a, b, c_or_null, w_dev, out, n, (hipStream_t)stream);
}

int afi_convT6s2_pack_weight(const float* w, float* wp, int Cin, int Cout, void* stream) {
    return afi_launch_convT_pack(w, wp, Cin, Cout, (hipStream_t)stream);
}
int afi_convT6s2_unpack_wgrad(const float* dwp, float* dw, int Cin, int Cout, void* stream) {
    return afi_launch_convT_unpack_grad(dwp, dw, Cin, Cout, (hipStream_t)stream);
}
static AfiPixGemm convT_fwd_desc(AfiView x, int N, int H, int W, int Cin, const float* wp, const float* bias, int Cout, AfiView out) {
    AfiPixGemm g = pix_default(N, H, W);
    g.Ck = Cin; g.Ncols = 4 * Cout; g.CoutPhase = Cout; g.o_up = 2;
    g.A = x; g.B = wp; g.b_sRow = 9LL * Cin; g.b_sTap = Cin;
    g.O = out; g.bias = bias;
    return g;
}
static AfiPixGemm convT_dgrad_desc(AfiView dy, int N, int H, int W, int Cout, const float* wp, int Cin, AfiView dx) {
    AfiPixGemm g = pix_default(N, H, W);
    g.a_sgn = -1; g.a_up = 2; g.nKphase = 4;
    g.Ck = Cout; g.Ncols = Cin; g.CoutPhase = Cin;
    g.A = dy; g.B = wp; g.b_sRow = 9LL * Cin; g.b_sTap = Cin;
    g.O = dx;
    return g;
}
static AfiWgradGemm convT_wgrad_desc(AfiView dy, AfiView x, int N, int H, int W, int Cout, int Cin, float* dwp, float alpha) {
    AfiWgradGemm g = conv_wgrad_desc(dy, x, N, H, W, 4 * Cout, Cin, dwp, alpha);
    g.dy_up = 2; g.CoutPhase = Cout;
    return g;
}
int afi_convT6s2_fwd(afi_ctx_t* ctx, afi_view_t x, int N, int H, int W, int Cin, const float* wp, const float* bias, int Cout, afi_view_t out, int lrelu,
                     void* stream) {
    afi_ctx* cx = ctx; (void)cx;
    AFI_CTX_CHECK(ctx);
    if ((Cout & 3) || (Cin & 3)) return AFI_ERR_UNSUPPORTED;
    AfiPixGemm g = convT_fwd_desc(V(x), N, H, W, Cin, wp, bias, Cout, V(out));
    g.lrelu = lrelu;
    return launch_pix_op(cx, g, 0, (hipStream_t)stream);
}
int afi_convT6s2_dgrad(afi_ctx_t* ctx, afi_view_t dy, int N, int H, int W, int Cout, const float* wp, int Cin, afi_view_t dx, afi_view_t z, void* stream) {
    afi_ctx* cx = ctx; (void)cx;
    AFI_CTX_CHECK(ctx);
    if ((Cout & 3) || (Cin & 3)) return AFI_ERR_UNSUPPORTED;
    AfiPixGemm g = convT_dgrad_desc(V(dy), N, H, W, Cout, wp, Cin, V(dx));
    if (z.p) { g.Z = V(z); g.z_lo = 0; g.z_hi = Cin; }
    return launch_pix_op(cx, g, 1, (hipStream_t)stream);
}
int afi_convT6s2_wgrad(afi_ctx_t* ctx, afi_view_t dy, afi_view_t x, int N, int H, int W, int Cout, int Cin, float* dwp, float alpha, void* stream) {
    afi_ctx* cx = ctx; (void)cx;
    AFI_CTX_CHECK(ctx);
    if ((Cout & 3) || (Cin & 3)) return AFI_ERR_UNSUPPORTED;
    return wgrad_launch(cx, convT_wgrad_desc(V(dy), V(x), N, H, W, Cout, Cin, dwp, alpha), (hipStream_t)stream);
}

int afi_bilinear2x_add_fwd(afi_view_t x, int N, int H, int W, int C, float beta, float* out, void* stream) {
    return afi_launch_bilinear2x_fwd(V(x), N, H, W, C, beta, out, (hipStream_t)stream);
}
int afi_bilinear2x_add_bwd(const float* dout, int N, int H, int W, int C, float beta, float* dx, void* stream) {
    return afi_launch_bilinear2x_bwd(dout, N, H, W, C, beta, dx, (hipStream_t)stream);
}
int afi_bn_stats(const float* x, long long P, int C, float* mean, float* invstd, float* var, float* rm, float* rv, float* scratch,
                 void* stream) {
    return afi_launch_bn_stats(x, P, C, mean, invstd, var, rm, rv, scratch, (hipStream_t)stream);
}
int afi_bn_apply_lrelu_fwd(const float* x, float* y, const float* mean, const float* invstd, const float* gamma, const float* beta,
                           long long P, int C, void* stream) {
    return afi_launch_bn_apply_lrelu(x, y, mean, invstd, gamma, beta, P, C, (hipStream_t)stream);
}
int afi_bn_stats_ex(const float* x, long long P, int C, float eps, float momentum, float* mean, float* invstd, float* var, float* rm, float* rv,
                    long long* nbt, float* scratch, void* stream) {
    if (eps < 0.f || momentum < 0.f || momentum > 1.f || !x || !mean || !invstd || !scratch || (rm == nullptr) != (rv == nullptr)) return AFI_ERR_BAD_ARG;
    return afi_launch_bn_stats(x, P, C, mean, invstd, var, rm, rv, scratch, (hipStream_t)stream, nbt, eps, momentum);
}
int afi_bn_apply_fwd(const float* x, float* y, const float* mean, const float* invstd, const float* gamma, const float* beta, long long P, int C,
                     float slope, void* stream) {
    return afi_launch_bn_apply_lrelu(x, y, mean, invstd, gamma, beta, P, C, (hipStream_t)stream, slope);
}
int afi_bn_bwd(const float* g, const float* x, float* dx, const float* mean, const float* invstd, const float* gamma, float* dgamma,
               float* dbeta, long long P, int C, float* scratch, void* stream) {
    return afi_launch_bn_bwd(g, x, dx, mean, invstd, gamma, dgamma, dbeta, 1.f, P, C, scratch, (hipStream_t)stream);
}
int afi_bn_bwd_sums(const float* g, const float* x, const float* mean, const float* invstd, float* dgamma, float* dbeta, float* sums2C, long long P, int C, float* scratch,
                    void* stream) {
    if (!g || !x || !mean || !invstd) return AFI_ERR_BAD_ARG;
    return afi_launch_bn_bwd_sums(g, x, mean, invstd, dgamma, dbeta, sums2C, P, C, scratch, (hipStream_t)stream);
}
int afi_bn_bwd_apply(const float* g, const float* x, float* dx, const float* mean, const float* invstd, const float* gamma, const float* sums2C, long long P,
                     long long P_total, int C, void* stream) {
    if (!g || !x || !dx || !mean || !invstd || !gamma) return AFI_ERR_BAD_ARG;
    return afi_launch_bn_bwd_apply(g, x, dx, mean, invstd, gamma, sums2C, P, P_total, C, (hipStream_t)stream);
}
int afi_colsum_accum(const float* g, long long P, int C, long long ld, float alpha, float* db, float* scratch, void* stream) {
    return afi_launch_colsum_accum(g, P, C, ld, alpha, db, scratch, (hipStream_t)stream);
}
int afi_bce_logits_fwd_bwd(const float* z, long long n, float target, float lscale, float* loss, float gscale, float* dz, void* stream) {
    return afi_launch_bce_logits(z, n, target, lscale, loss, gscale, dz, (hipStream_t)stream);
}
int afi_l1_fwd_bwd(afi_view_t a, afi_view_t b, int N, int h, int w, int C, int Ha, int Wa, float lscale, float* loss, float gscale,
                   float* da, void* stream) {
    return afi_launch_l1(V(a), V(b), N, h, w, C, Ha, Wa, lscale, loss, gscale, da, (hipStream_t)stream);
}
int afi_sgd_momentum_step(const afi_sgd_desc_t* descs_dev, int ntensors, long long max_n, float lr, float momentum, float gscale,
                          void* stream) {
    return afi_launch_sgd(descs_dev, ntensors, max_n, lr, momentum, gscale, (hipStream_t)stream);
}
int afi_scale_inplace(float* p, long long n, float s, void* stream) { return afi_launch_scale(p, n, s, (hipStream_t)stream); }
int afi_nchw_to_nhwc(const float* in, float* out, int N, int C, int P, void* stream) {
    return afi_launch_nchw_to_nhwc(in, out, N, C, P, (hipStream_t)stream);
}
int afi_nhwc_to_nchw(const float* in, float* out, int N, int C, int P, void* stream) {
    return afi_launch_nhwc_to_nchw(in, out, N, C, P, (hipStream_t)stream);
}
int afi_cast_to_f32_nhwc(const void* src, int src_dtype, int N, int C, int H, int W, long long sN, long long sC, long long sH, long long sW, float* dst,
                         void* stream) {
    return afi_launch_cast_to_f32_nhwc(src, src_dtype, N, C, H, W, sN, sC, sH, sW, dst, (hipStream_t)stream);
}
int afi_cast_from_f32_nhwc(afi_view_t src, int N, int H, int W, int C, void* dst, int dst_dtype, void* stream) {
    return afi_launch_cast_from_f32_nhwc(V(src), N, H, W, C, dst, dst_dtype, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------------ generator
// forward workspace layout (floats):  [Wp 36*C*C][buf_r : n_rdb x P*L][t : P*C][a7 : P*C][u : 4P*C]     L = C + 4G
// split-K scratch shared by the GEMMs of one call (they run one after the other on the caller's stream): small maps get
// room for 16 slabs of the largest layer, capped at 18 MB; mid-size maps (< 1536 tiles of 128x128, launch_pix's second rule)
// 4 slabs of the largest layer (at most 4 x 25 M floats = 400 MB)
static long long part_floats(std::initializer_list<long long> layer_mn) {   // M x Ncols of every GEMM output of the call
    const long long cap = 4608LL * 1024;
    long long want = 0;
    for (long long mn : layer_mn) {
        const long long small = 16 * mn < cap ? 16 * mn : cap;
        if (small > want) want = small;
        if (mn < 1536LL * 128 * 128 && 4 * mn > want) want = 4 * mn;
    }
    return align4(want);
}
// Winograd scratch of one interpolator call: the largest of its eligible convs (C->C and L->C on the low-res grid, the
// conv-transpose as C->4C, C->C on the hi-res grid); 0 when nothing is eligible (small maps / few channels)
static long long gen_wino_floats(int C, int L, int N, int H, int W) {
    if (C < 128) return 0;
    long long m = 0;
    auto upd = [&](long long v) { if (v > m) m = v; };
    if ((long long)N * H * W >= 1024) { upd(wino_ws_floats(N, H, W, C, C)); upd(wino_ws_floats(N, H, W, L, C)); upd(wino_ws_floats(N, H, W, C, 4 * C)); }
    if (4LL * N * H * W >= 1024) upd(wino_ws_floats(N, 2 * H, 2 * W, C, C));
    return m;
}
struct GenWs {
    long long P, L;
    long long o_wp, o_buf, o_t, o_a7, o_u, o_part, n_part, o_wino, n_wino, o_rdbx, n_rdbx, o_img, n_img, total;
};
static GenWs gen_ws(int C, int G, int n_rdb, int N, int H, int W) {
    GenWs w;
    w.P = (long long)N * H * W; w.L = C + 4LL * G;
    long long o = 0;
    w.o_wp = o; o += align4(36LL * C * C);
    w.o_buf = o; o += align4((long long)n_rdb * w.P * w.L);
    w.o_t = o; o += align4(w.P * C);
    w.o_a7 = o; o += align4(w.P * C);
    w.o_u = o; o += align4(4 * w.P * C);
    w.n_part = part_floats({w.P * C, 4 * w.P * C});
    w.o_part = o; o += w.n_part;
    w.n_wino = gen_wino_floats(C, (int)w.L, N, H, W);
    w.o_wino = o; o += w.n_wino;
    w.n_rdbx = align4(4LL * G * 9 * C);                   // the growth convs' weights on the block input, packed [4G][3][3][C] (when no cache holds them)
    w.o_rdbx = o; o += (long long)n_rdb * w.n_rdbx;
    w.n_img = gen_wk6_fwd_floats(C, G, n_rdb, w.P);         // small maps: bf16x6 weight images of the forward GEMMs (when no weight cache holds them)
    w.o_img = o; o += w.n_img;
    w.total = o;
    return w;
}
long long afi_generator_fwd_ws_floats(int C, int G, int n_rdb, int N, int H, int W) { return gen_ws(C, G, n_rdb, N, H, W).total; }

// backward scratch layout: [dU 4P*C][gA P*C][gB P*C][dBuf P*L per RDB][dWp 36*C*C][red]
struct GenBwdWs {
    long long o_du, o_ga, o_gb, o_db0, o_dwp, o_rdbw, n_rdbw, o_rdbx, n_rdbx, o_red, o_part, n_part, o_wino, n_wino, o_wino2, o_img, n_img, total;
};
static GenBwdWs gen_bwd_ws(int C, int G, int n_rdb, int N, int H, int W) {
    GenBwdWs w;
    const long long P = (long long)N * H * W, L = C + 4LL * G;
    long long o = 0;
    w.o_du = o; o += align4(4 * P * C);
    w.o_ga = o; o += align4(P * C);
    w.o_gb = o; o += align4(P * C);
    w.o_db0 = o; o += align4((long long)n_rdb * P * L);      // one gradient buffer per RDB: no reuse, so the side-stream wgrads never race a later write
    w.o_dwp = o; o += align4(36LL * C * C);
    w.n_rdbw = align4(4LL * G * 9 * L);                   // packed weight gradient of a dense block's four growth convs (one per block:
    w.o_rdbw = o; o += (long long)n_rdb * w.n_rdbw;       //  the side stream may still be unpacking block r while block r - 1 is filled)
    w.n_rdbx = align4(4LL * G * 9 * C);                   // the growth convs' weights on the block input, packed [4G][3][3][C] (when no cache holds them)
    w.o_rdbx = o; o += (long long)n_rdb * w.n_rdbx;
    w.o_red = o; o += align4(afi_reduce_scratch_floats(C));
    w.n_part = part_floats({P * C, P * L, 4 * P * C});
    w.o_part = o; o += w.n_part;
    w.n_wino = gen_wino_floats(C, (int)L, N, H, W);
    w.o_wino = o; o += w.n_wino;                          // data-gradient chain (main stream)
    w.o_wino2 = o; o += w.n_wino;                         // weight gradients (side stream on small maps)
    w.n_img = gen_wk6_bwd_floats(C, G, n_rdb, P);           // small maps: bf16x6 weight images of the data-gradient GEMMs
    w.o_img = o; o += w.n_img;
    w.total = o;
    return w;
}
long long afi_generator_bwd_ws_floats(int C, int G, int n_rdb, int N, int H, int W) { return gen_bwd_ws(C, G, n_rdb, N, H, W).total; }

static int gen_check(const afi_gen_params_t* p) {
    if (!p || p->C <= 0 || p->G <= 0 || p->n_rdb < 1 || p->n_rdb > AFI_MAX_RDB) return AFI_ERR_BAD_ARG;
    if ((p->C & 3) || (p->G & 3)) return AFI_ERR_UNSUPPORTED;
    return AFI_OK;
}

// ---- Which schedule an interpolator call runs: every choice either pass makes, decided once from the context's options and arithmetic and the
// call's shape (DESIGN.md 4 has the table).  generator_fwd and afi_generator_bwd build the plan at their top and read it.  The two passes need
// not choose alike: every schedule of the forward leaves the same activations in the same layout, whatever the backward then runs.
struct GenPlan {
    GenWs ws;          // the forward's workspace (the backward reads the activations and the packed conv-transpose weight from it)
    GenBwdWs bws;      // the backward's scratch
    // the final conv on the up-sampled map (4x the pixels) and its data gradient stay on the small-map kernel, on a weight image, where a pass
    // builds images at all: at config 1 (50 x 68) the Winograd form is five launches of 9 .. 19 us
    bool hires_wk6;
    struct Fwd {
        // the dense block in COLUMN-BATCHED form: conv_k reads cat(x, y1 .. y_{k-1}); instead of five convs whose K grows (and whose four
        // 32-column outputs are 27 tiles each, for 256 CUs), five steps whose source is ONE slice: step 0 multiplies x into the columns of all
        // five convs in one grouped launch (384 columns, K = 9*C), step j = 1..4 multiplies y_j (32 channels, K = 288) into the convs that still
        // need it; a conv's slice accumulates in place (beta = 1) and is activated by the step that completes it.  Same multiply-adds as
        // generator_rdb.py:64-71, summed in another order (fp32 rounding only).  AFI_OPT_G_SMALLMAP_MAX_PIXELS = 0 (and, under the six-product
        // arithmetics, AFI_OPT_G_SMALLMAP6_MAX_PIXELS = 0): conv by conv at every size.
        bool batched;
        // the batched form ON WEIGHT IMAGES: its GEMMs, the head / trunk convs and the conv-transpose run on the bf16 matrix cores in the
        // six-product form, on pre-split weight images (csrc/smallmap.hip).  Asks the arithmetic (bf16x6 / f16x3) and shapes the images take
        // (GenWs::n_img > 0); AFI_OPT_DETERMINISTIC does not matter here.  Not Bwd::six: that one is about the weight gradients
        bool six;
        // larger maps: what the four growth convs take from the block input x is ONE conv C -> 4G on the packed weights [4G][3][3][C]
        // (Winograd-eligible at the reference's widths; the per-conv form runs four 32-column direct GEMMs 2304+ deep), stored as raw partial
        // sums in their four slices; conv_k then adds what it takes from y_1 .. y_{k-1} ((k-1) G channels) and activates.  Same multiply-adds,
        // another order.  (4G <= C: the Winograd scratch is sized for C -> C; every shape of the reference has G = 32, C = 256.)
        // Deliberately not Bwd::batch_growth's test: this one asks P > AFI_OPT_G_GROUPED_WGRAD_MAX_PIXELS, that one !Bwd::grouped, so a
        // deterministic call at or below that size runs conv by conv forward and batched backward
        bool xbatch;
        // value 16 of AFI_OPT_WINOGRAD_F4_FORWARD: the interpolator's own Winograd forwards on F(4x4) as well -- measured, off: DESIGN.md 9
        bool f4;
    } fwd;
    struct Bwd {
        // Small maps (config-1 sizes): every weight / bias gradient is DEFERRED to the end of the pass and runs as ONE grouped launch per tile
        // shape (csrc/smallmap.hip: whole dW tiles per block, no split over pixels, no atomics, no zero-fill), instead of one 7 .. 36-tile
        // launch per layer on a side stream.  All their operands (dOut, dU, gA, gB, the per-block gradient buffers and the saved activations)
        // stay alive until the call returns.  AFI_OPT_G_GROUPED_WGRAD_MAX_PIXELS = 0 (and AFI_OPT_G_SMALLMAP6_MAX_PIXELS = 0) restores the
        // per-layer launches, and so does AFI_OPT_DETERMINISTIC: the grouped stream-K launches add the tiles two runs share by atomics.
        // Deliberately not Fwd::batched's test: other options, `<=` where that one has `<`, and the forward does not look at `deterministic`
        bool grouped;
        // the grouped weight gradients on the bf16 matrix cores in the six-product form (csrc/smallmap.hip): grouped, under bf16x6 / f16x3
        bool six;
        // the data-gradient GEMMs on pre-split weight images: `six`, and shapes the images take (GenBwdWs::n_img > 0)
        bool images;
        // under `six` the four growth convs' weight gradients of a block run as ONE 4G-row problem dy[C : C + 4G] (x) cat[0 : L] into a packed
        // [4G][3][3][L] buffer (1.26x their products, on the 128 x 128 tile of that kernel instead of four 32-row problems on the fp32 one),
        // unpacked after the group launch -- the grouped form of batch_growth
        bool pack_growth;
        // larger maps (per-layer form): a block's four growth-conv weight gradients as one packed GEMM, and what their data gradients leave on
        // the block input as one 4G -> C data gradient (gen_bwd_block)
        bool batch_growth;
        // the per-layer weight / bias gradients beside the data-gradient chain, on the context's side stream.  Not in the grouped form: flushing
        // the deferred problems onto the side stream after the hi-res pair, after each dense block and at the end was measured: the grouped
        // launches then run beside the chain, every kernel of which gets slower by about what is gained (1.26 vs 1.19 ms eager, and 1.51 ms
        // replayed from a hipGraph with its six fork/join edges): the chain's kernels already occupy every CU even where they wait on memory
        bool side_stream;
        // the packed conv-transpose gradient and the packed growth-conv gradients are neighbours in the scratch: ONE zero fill for both (the
        // layout's part of the test; the call adds that the conv-transpose gradient is asked for, and the pointer's alignment)
        bool one_fill;
    } bwd;
};
constexpr int kGenWideMax = 4 + 2 * AFI_MAX_RDB;    // wide weight-gradient problems of one grouped backward pass with packed growth gradients
static GenPlan gen_plan(const afi_ctx* cx, int C, int G, int R, int N, int H, int W) {
    GenPlan p;
    p.ws = gen_ws(C, G, R, N, H, W);
    p.bws = gen_bwd_ws(C, G, R, N, H, W);
    const long long P = p.ws.P;
    const bool dt6 = afi_dtype_smallmap6(cx ? cx->dtype : afi_default_dtype());
    const bool growth = afi_opt(cx, AFI_OPT_G_BATCH_GROWTH_GRADS) != 0 && (4 * G <= C || p.ws.n_wino == 0);   // (n_wino: the same in both layouts)
    p.hires_wk6 = 4 * P <= kWk6HiResMaxPixels;
    const bool img6 = dt6 && p.ws.n_img > 0;
    p.fwd.batched = P < afi_opt(cx, AFI_OPT_G_SMALLMAP_MAX_PIXELS) || (img6 && P <= afi_opt(cx, AFI_OPT_G_SMALLMAP6_MAX_PIXELS));
    p.fwd.six = p.fwd.batched && img6;
    p.fwd.xbatch = !p.fwd.batched && P > afi_opt(cx, AFI_OPT_G_GROUPED_WGRAD_MAX_PIXELS) && growth;
    p.fwd.f4 = (afi_opt(cx, AFI_OPT_WINOGRAD_F4_FORWARD) & 16) != 0;
    p.bwd.grouped = !afi_det(cx) && (P <= afi_opt(cx, AFI_OPT_G_GROUPED_WGRAD_MAX_PIXELS) || (dt6 && p.bws.n_img > 0 && P <= afi_opt(cx, AFI_OPT_G_SMALLMAP6_MAX_PIXELS)));
    p.bwd.six = p.bwd.grouped && dt6;
    p.bwd.images = p.bwd.six && p.bws.n_img > 0;
    p.bwd.pack_growth = p.bwd.six;                         // (its 4 + 2 R wide problems fit the deferred table: kGenWideMax)
    p.bwd.batch_growth = !p.bwd.grouped && growth;
    p.bwd.side_stream = !p.bwd.grouped && 4 * P <= kSideStreamMaxPixels;
    p.bwd.one_fill = p.bwd.pack_growth && p.bws.o_rdbw == p.bws.o_dwp + align4(36LL * C * C) && (p.bws.n_rdbw & 3) == 0;
    return p;
}
// the weight gradient of a 3x3 conv co <- ci in Winograd form: both channel counts and the map large enough, and the scratch (sized by
// gen_wino_floats for the call's C -> C, L -> C and C -> 4C convs) holds what this one needs
static bool gen_wino_wgrad_ok(const afi_ctx* cx, const GenPlan& p, int co, int ci, long long pixels, long long need_floats = 0) {
    return p.bws.n_wino > 0 && p.bws.n_wino >= need_floats && co >= 128 && ci >= 128 && pixels >= wino_g_minpix(cx) && afi_opt(cx, AFI_OPT_WINOGRAD) != 0;
}
// One pixel GEMM of a pass (forward conv or data gradient): Winograd where the conv is eligible and no weight image is attached, else the
// direct kernels with the call's split-K scratch.  wino / part: in the pass's own workspace; f4: GenPlan::Fwd::f4 (the forward only)
struct GenPix {
    afi_ctx* cx; float* wino; long long n_wino; float* part; long long n_part; bool f4; hipStream_t st;
    int operator()(AfiPixGemm g, int b_rc) const {
        if (!g.Bimg && n_wino > 0 && wino_eligible(cx, g, b_rc)) return wino_run(cx, g, wino_form(cx, g, b_rc, f4), wino, n_wino, part, n_part, st);
        g.partial = part; g.partial_floats = n_part;
        return afi_launch_pix_gemm(g, b_rc, st);
    }
};
// the weight images of a pass on images (Fwd::six / Bwd::images), in wk6_build's order; returns their number (5 R + 4 at most: kWk6MaxReq).
// wp: the packed fp32 conv-transpose weight, written by further blocks of the image launch (the pack used to be a launch of its own)
static int gen_fwd_image_reqs(const GenPlan& p, const afi_gen_params_t* prm, float* wp, Wk6Req* rq) {
    const int C = prm->C, G = prm->G, L = (int)p.ws.L;
    int nr = 0;
    rq[nr++] = wk6_req(prm->w0, prm->w0, C, C, 1, 0, 9LL * C, C);
    for (int r = 0; r < prm->n_rdb; ++r) {
        for (int k = 1; k <= 4; ++k) { const int cin = C + (k - 1) * G; rq[nr++] = wk6_req(prm->rdb_w[r][k - 1], prm->rdb_w[r][k - 1], G, cin, 1, 0, 9LL * cin, cin); }
        rq[nr++] = wk6_req(prm->rdb_w[r][4], prm->rdb_w[r][4], C, L, 1, 0, 9LL * L, L);
    }
    rq[nr++] = wk6_req(prm->w7, prm->w7, C, C, 1, 0, 9LL * C, C);
    rq[nr] = wk6_req(prm->wT, prm->wT, 4 * C, C, 1, 0, 9LL * C, C);    // the conv-transpose image straight from the parameter's own layout
    rq[nr].convT = 1; rq[nr].pack_dst = wp; ++nr;
    if (p.hires_wk6) rq[nr++] = wk6_req(prm->w9, prm->w9, C, C, 1, 0, 9LL * C, C);
    return nr;
}
static int gen_bwd_image_reqs(const GenPlan& p, const afi_gen_params_t* prm, bool want_dx, Wk6Req* rq) {
    const int C = prm->C, G = prm->G, L = (int)p.ws.L;
    int nr = 0;
    rq[nr] = wk6_req(prm->wT, prm->wT, C, C, 4, 1, 9LL * C, C);        // conv-transpose data gradient: K = (Cout chunk, phase, tap), straight from the parameter's layout
    rq[nr].convT = 2; ++nr;
    rq[nr++] = wk6_req(prm->w7, prm->w7, C, C, 1, 1, 9LL * C, C);
    for (int r = 0; r < prm->n_rdb; ++r) {
        rq[nr++] = wk6_req(prm->rdb_w[r][4], prm->rdb_w[r][4], L, C, 1, 1, 9LL * L, L);
        for (int k = 1; k <= 4; ++k) { const int cin = C + (k - 1) * G; rq[nr++] = wk6_req(prm->rdb_w[r][k - 1], prm->rdb_w[r][k - 1], cin, G, 1, 1, 9LL * cin, cin); }
    }
    if (want_dx) rq[nr++] = wk6_req(prm->w0, prm->w0, C, C, 1, 1, 9LL * C, C);
    if (p.hires_wk6) rq[nr++] = wk6_req(prm->w9, prm->w9, C, C, 1, 1, 9LL * C, C);
    return nr;
}

// out_dtype (AFI_STORE_*): storage of `out` only -- the final conv's epilogue rounds there; everything before it is fp32
static int generator_fwd(afi_ctx_t* cx, const afi_gen_params_t* prm, afi_view_t xv, int N, int H, int W, afi_view_t outv, int out_dtype, float* ws,
                         long long ws_floats, void* stream) {
    AFI_CTX_CHECK(cx);
    AFI_TRY(gen_check(prm));
    if (N <= 0 || H <= 0 || W <= 0 || !ws || !xv.p || !outv.p) return AFI_ERR_BAD_ARG;
    if (out_dtype != AFI_STORE_F32 && out_dtype != AFI_STORE_BF16 && out_dtype != AFI_STORE_F16) return AFI_ERR_BAD_ARG;
    const int C = prm->C, G = prm->G, R = prm->n_rdb;
    const GenPlan p = gen_plan(cx, C, G, R, N, H, W);
    const GenWs& l = p.ws;
    if (ws_floats < l.total) return AFI_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const GenPix PG{cx, ws + l.o_wino, l.n_wino, ws + l.o_part, l.n_part, p.fwd.f4, st};
    const int L = (int)l.L;
    const float rs = prm->residual_scale;
    float* wp = ws + l.o_wp;
    AfiView x = V(xv);
    auto buf = [&](int r) { return dense_view(ws + l.o_buf + (long long)r * l.P * L, H, W, L); };
    AfiView t = dense_view(ws + l.o_t, H, W, C), a7 = dense_view(ws + l.o_a7, H, W, C);
    AfiView u = dense_view(ws + l.o_u, 2 * H, 2 * W, C);

    Wk6Images im;
    bool packed = false;                                   // the packed conv-transpose weight `wp` (the backward reads it from this workspace) exists
    if (p.fwd.six) {
        Wk6Req rq[kWk6MaxReq];
        AFI_TRY(wk6_build(cx, im, rq, gen_fwd_image_reqs(p, prm, wp, rq), ws + l.o_img, l.n_img, st, nullptr, nullptr, &packed));
    }
    if (!packed) {   // packed conv-transpose weight: from the caller's weight cache when one is registered (BiFPN: 28 calls on one set of weights)
        bool hit = false;
        const long long wp_floats = 36LL * C * C;
        if (float* slot = wino_wcache_slot(cx, prm->wT, /*tag: convT pack*/ 2, 0, C, C, align4(wp_floats), hit)) {
            if (!hit) AFI_TRY(afi_launch_convT_pack(prm->wT, slot, C, C, st));
            if (hipMemcpyAsync(wp, slot, sizeof(float) * wp_floats, hipMemcpyDeviceToDevice, st) != hipSuccess) return AFI_ERR_LAUNCH;
        } else {
            AFI_TRY(afi_launch_convT_pack(prm->wT, wp, C, C, st));
        }
    }
    {   // the f16x3 weight images of the pass's Winograd convs that the cache does not hold yet, in one builder call: the convs below, in their
        // order, by the fields wino_eligible and wino_form read.  The growth convs' packed x-part takes its cache slot (and is packed) here,
        // where the walk meets it: the block below then finds it
        WinoImgBatch ib(cx);
        auto want = [&](AfiPixGemm g, const float* key, int c_lo = 0) { if (key) im.attach(g, key, c_lo); ib.add(g, 0, l.n_wino, p.fwd.f4); };
        want(conv_fwd_desc(x, N, H, W, C, prm->w0, prm->b0, C, buf(0)), prm->w0);
        for (int r = 0; r < R && !p.fwd.batched && ib.open; ++r) {
            if (p.fwd.xbatch) {
                const float* const wk[4] = {prm->rdb_w[r][0], prm->rdb_w[r][1], prm->rdb_w[r][2], prm->rdb_w[r][3]};
                bool hit = false;
                if (float* slot = wino_wcache_slot(cx, prm->rdb_w[r][0], /*tag: growth x-part pack*/ 3, 0, 4 * G, C, l.n_rdbx, hit)) {
                    if (!hit) AFI_TRY(afi_launch_rdb_xpart_pack(wk, slot, C, G, st));
                    want(conv_fwd_desc(buf(r), N, H, W, C, slot, nullptr, 4 * G, ch_off(buf(r), C)), nullptr);
                }
            } else {
                for (int k = 1; k <= 4; ++k) want(conv_fwd_desc(buf(r), N, H, W, C + (k - 1) * G, prm->rdb_w[r][k - 1], nullptr, G, buf(r)), nullptr);
            }
            want(conv_fwd_desc(buf(r), N, H, W, L, prm->rdb_w[r][4], nullptr, C, buf(r)), prm->rdb_w[r][4]);
        }
        // (the column-batched blocks run as grouped launches on the small-map kernels: no Winograd conv among them)
        want(conv_fwd_desc(t, N, H, W, C, prm->w7, prm->b7, C, a7), prm->w7);
        want(convT_fwd_desc(a7, N, H, W, C, wp, prm->bT, C, u), prm->wT);
        want(conv_fwd_desc(u, N, 2 * H, 2 * W, C, prm->w9, prm->b9, C, V(outv)), prm->w9);
        AFI_TRY(ib.build(ws + l.o_wino, st));
    }
    {   // head conv + LReLU (generator_rdb.py:91-93) -> channels [0,C) of RDB 0's dense buffer
        AfiPixGemm g = conv_fwd_desc(x, N, H, W, C, prm->w0, prm->b0, C, buf(0));
        g.lrelu = 1;
        im.attach(g, prm->w0);
        AFI_TRY(PG(g, 0));
    }
    for (int r = 0; r < R; ++r) {   // ResidualDenseBlock.forward (generator_rdb.py:64-71); the dense buffer replaces torch.cat
        AfiView b = buf(r);
        const bool last = (r == R - 1);
        // conv5 restricted to input channels [c_lo, c_lo + nch); on the channels from c_lo = 0 ride the residual terms (no activation follows conv5):
        // x + rs * conv5, and behind the last block ResidualInResidual.forward (:27-30): rs*(x + rs*conv5) + a0
        auto conv5_desc = [&](int c_lo, int nch) {
            AfiPixGemm g = conv_fwd_desc(ch_off(b, c_lo), N, H, W, nch, prm->rdb_w[r][4] + c_lo, nullptr, C, last ? t : buf(r + 1));
            g.b_sRow = 9LL * L; g.b_sTap = L;
            g.alpha = last ? rs * rs : rs;
            if (c_lo == 0) {
                g.R1 = b; g.r1_lo = 0; g.r1_hi = C; g.r1s = last ? rs : 1.f;
                if (last) { g.R2 = buf(0); g.r2s = 1.f; g.r2_lo = 0; g.r2_hi = C; }
            } else {
                g.beta = 1.f;
            }
            im.attach(g, prm->rdb_w[r][4], c_lo);
            return g;
        };
        if (p.fwd.batched) {
            for (int j = 0; j <= 4; ++j) {              // source slice j: x (j = 0) or y_j
                const int c_lo = j == 0 ? 0 : C + (j - 1) * G, nch = j == 0 ? C : G;
                AfiPixGemm probs[5];
                int n = 0;
                for (int k = j + 1; k <= 4; ++k) {      // growth conv k, its input channels [c_lo, c_lo + nch)
                    const int cin = C + (k - 1) * G;
                    AfiPixGemm g = conv_fwd_desc(ch_off(b, c_lo), N, H, W, nch, prm->rdb_w[r][k - 1] + c_lo, nullptr, G, ch_off(b, cin));
                    g.b_sRow = 9LL * cin; g.b_sTap = cin;
                    g.beta = j == 0 ? 0.f : 1.f;
                    g.lrelu = (k == j + 1) ? 1 : 0;     // this step completes conv_k
                    im.attach(g, prm->rdb_w[r][k - 1], c_lo);
                    probs[n++] = g;
                }
                probs[n++] = conv5_desc(c_lo, nch);
                const int rc = afi_launch_pix_gemm_group(probs, n, 0, st);
                if (rc == AFI_ERR_UNSUPPORTED) { for (int i = 0; i < n; ++i) AFI_TRY(PG(probs[i], 0)); }   // same step, one launch per conv
                else AFI_TRY(rc);
            }
            continue;
        }
        if (p.fwd.xbatch) {
            const float* const wk[4] = {prm->rdb_w[r][0], prm->rdb_w[r][1], prm->rdb_w[r][2], prm->rdb_w[r][3]};
            float* Wx = ws + l.o_rdbx + (long long)r * l.n_rdbx;
            bool hit = false, scratch_b = true;
            if (float* slot = wino_wcache_slot(cx, prm->rdb_w[r][0], /*tag: growth x-part pack*/ 3, 0, 4 * G, C, l.n_rdbx, hit)) { Wx = slot; scratch_b = false; }
            if (!hit) AFI_TRY(afi_launch_rdb_xpart_pack(wk, Wx, C, G, st));
            AfiPixGemm ga = conv_fwd_desc(b, N, H, W, C, Wx, nullptr, 4 * G, ch_off(b, C));
            ga.no_wcache = scratch_b ? 1 : 0;
            AFI_TRY(PG(ga, 0));
            AFI_TRY(afi_launch_lrelu_slice(ch_off(b, C), N, H, W, G, st));          // conv_1 takes nothing else: its slice is complete
            for (int k = 2; k <= 4; ++k) {
                const int cin = C + (k - 1) * G;
                AfiPixGemm g = conv_fwd_desc(ch_off(b, C), N, H, W, cin - C, prm->rdb_w[r][k - 1] + C, nullptr, G, ch_off(b, cin));
                g.b_sRow = 9LL * cin; g.b_sTap = cin;                   // (a column range of the [G][3][3][cin] weight)
                g.beta = 1.f; g.lrelu = 1;
                AFI_TRY(PG(g, 0));
            }
        } else
        for (int k = 1; k <= 4; ++k) {
            const int cin = C + (k - 1) * G;
            AfiPixGemm g = conv_fwd_desc(b, N, H, W, cin, prm->rdb_w[r][k - 1], nullptr, G, ch_off(b, cin));
            g.lrelu = 1;
            AFI_TRY(PG(g, 0));
        }
        AFI_TRY(PG(conv5_desc(0, L), 0));
    }
    {   // trunk conv + LReLU (:97-99)
        AfiPixGemm g = conv_fwd_desc(t, N, H, W, C, prm->w7, prm->b7, C, a7);
        g.lrelu = 1;
        im.attach(g, prm->w7);
        AFI_TRY(PG(g, 0));
    }
    {   // ConvTranspose2d k6 s2 p2 + LReLU (:101-105) as a 4-phase 3x3 conv with a pixel-shuffle store
        AfiPixGemm g = convT_fwd_desc(a7, N, H, W, C, wp, prm->bT, C, u);
        g.lrelu = 1;
        im.attach(g, prm->wT);
        AFI_TRY(PG(g, 0));
    }
    {   // final conv (:107-108) + bilinear x2 skip of the input (:125,130) fused in the epilogue
        AfiPixGemm g = conv_fwd_desc(u, N, 2 * H, 2 * W, C, prm->w9, prm->b9, C, V(outv));
        g.R1 = x; g.r1s = 1.f; g.r1_lo = 0; g.r1_hi = C; g.r1_bilinear = 1;
        g.o_dtype = out_dtype;
        im.attach(g, prm->w9);                              // (GenPlan::hires_wk6 only: no image was requested otherwise)
        AFI_TRY(PG(g, 0));
    }
    return AFI_OK;
}

int afi_generator_fwd(afi_ctx_t* ctx, const afi_gen_params_t* prm, afi_view_t xv, int N, int H, int W, afi_view_t outv, float* ws, long long ws_floats,
                      void* stream) {
    return generator_fwd(ctx, prm, xv, N, H, W, outv, AFI_STORE_F32, ws, ws_floats, stream);
}
int afi_generator_fwd_out16(afi_ctx_t* ctx, const afi_gen_params_t* prm, afi_view_t xv, int N, int H, int W, afi_view_t outv, int out_dtype, float* ws,
                            long long ws_floats, void* stream) {
    if (out_dtype != AFI_STORE_BF16 && out_dtype != AFI_STORE_F16) return AFI_ERR_BAD_ARG;
    return generator_fwd(ctx, prm, xv, N, H, W, outv, out_dtype, ws, ws_floats, stream);
}

// The weight / bias gradients a grouped backward (GenPlan::Bwd::grouped) puts off to its end: one grouped launch per tile shape, then ONE tail
// launch for the bias gradients, the conv-transpose gradient's unpack and every packed growth-conv gradient.  All on the caller's stream.
struct GenDeferred {
    AfiWgradGemm wide[kGenWideMax], narrow[4 * AFI_MAX_RDB];
    AfiColsumProb cs[8];                                   // (the pass has four biases)
    int n_wide = 0, n_narrow = 0, n_cs = 0;
    bool convT = false;                                    // the conv-transpose gradient (packed, in GenBwdWs::o_dwp) is among them
    unsigned packed_mask = 0;                              // dense blocks whose packed growth-conv gradient (GenBwdWs::o_rdbw) is among them
    int defer(const afi_ctx* cx, const AfiWgradGemm& g, hipStream_t st) {
        if (g.Mrows <= 32 && n_narrow < 4 * AFI_MAX_RDB) { narrow[n_narrow++] = g; return AFI_OK; }
        if (g.Mrows > 32 && n_wide < kGenWideMax) { wide[n_wide++] = g; return AFI_OK; }
        return wgrad_launch(cx, g, st);                    // table full (unusual shapes): launch it on its own
    }
    void defer(const float* g, long long rows, int Cc, long long ld, float* db) { cs[n_cs++] = AfiColsumProb{g, db, rows, ld, Cc, 1.f}; }
    int flush(const GenPlan& p, const afi_gen_params_t* prm, const afi_gen_params_t* gr, float* scratch, hipStream_t st) {
        if (n_wide + n_narrow + n_cs == 0 && !convT) return AFI_OK;
        const int rc6 = p.bwd.six ? afi_launch_wgrad_gemm_group6(wide, n_wide, st) : AFI_ERR_UNSUPPORTED;     // (unsupported: nothing was launched)
        AFI_TRY(rc6 == AFI_ERR_UNSUPPORTED ? afi_launch_wgrad_gemm_group(wide, n_wide, 1, st) : rc6);
        AFI_TRY(afi_launch_wgrad_gemm_group(narrow, n_narrow, 0, st));
        const int C = prm->C, R = prm->n_rdb;
        float* dws[AFI_MAX_RDB][4];                        // (a block that was not packed: null targets)
        for (int r = 0; r < R; ++r)
            for (int k = 0; k < 4; ++k) dws[r][k] = (packed_mask >> r & 1) ? gr->rdb_w[r][k] : nullptr;
        return afi_launch_g_bwd_tail(cs, n_cs, convT ? scratch + p.bws.o_dwp : nullptr, gr->wT, C, C, scratch + p.bws.o_rdbw, p.bws.n_rdbw, dws, packed_mask ? R : 0,
                                     C, prm->G, 1.f, st);
    }
};
// what the steps of one backward call share
struct GenBwd {
    afi_ctx* cx; const GenPlan& p; const afi_gen_params_t *prm, *gr; int N, H, W; const float* ws; float* scratch; hipStream_t st;
    GenPix PG;
    Fork fk;                                               // fk.side: weight / bias gradients of the per-layer form (Bwd::side_stream; else the main stream)
    GenDeferred df;
    Wk6Images im;                                          // weight images of the data-gradient GEMMs (row-contiguous weights)
    // (a constructor, not aggregate initialisation: that would zero the deferred tables, 8 KB per call)
    GenBwd(afi_ctx* cx_, const GenPlan& p_, const afi_gen_params_t* prm_, const afi_gen_params_t* gr_, int N_, int H_, int W_, const float* ws_, float* scratch_, hipStream_t st_)
        : cx(cx_), p(p_), prm(prm_), gr(gr_), N(N_), H(H_), W(W_), ws(ws_), scratch(scratch_), st(st_),
          PG{cx_, scratch_ + p_.bws.o_wino, p_.bws.n_wino, scratch_ + p_.bws.o_part, p_.bws.n_part, false, st_}, fk(cx_, st_, p_.bwd.side_stream) {}
    AfiView buf(int r) const { return dense_view(ws + p.ws.o_buf + (long long)r * p.ws.P * p.ws.L, H, W, p.ws.L); }               // saved dense buffer of RDB r
    AfiView dbuf(int r) const { return dense_view(scratch + p.bws.o_db0 + (long long)r * p.ws.P * p.ws.L, H, W, p.ws.L); }        // its gradient
    // weight gradient of a 3x3 conv (h x w: the low-res or the up-sampled map): deferred, or Winograd F(3x3,2x2) where gen_wino_wgrad_ok, or direct
    int wgrad(AfiView dy, AfiView xin, int h, int w, int co, int ci, float* dw, float alpha) {
        if (p.bwd.grouped) return df.defer(cx, conv_wgrad_desc(dy, xin, N, h, w, co, ci, dw, alpha), st);
        if (gen_wino_wgrad_ok(cx, p, co, ci, (long long)N * h * w)) return wino_wgrad(cx, dy, xin, N, h, w, co, ci, dw, alpha, scratch + p.bws.o_wino2, p.bws.n_wino, fk.side);
        return wgrad_launch(cx, conv_wgrad_desc(dy, xin, N, h, w, co, ci, dw, alpha), fk.side);
    }
    int colsum(const float* g, long long rows, int Cc, long long ld, float* db) {      // bias gradient
        if (p.bwd.grouped) { df.defer(g, rows, Cc, ld, db); return AFI_OK; }
        return afi_launch_colsum_accum(g, rows, Cc, ld, 1.f, db, scratch + p.bws.o_red, fk.side);
    }
};
// One dense block backwards (generator_rdb.py:64-71).  Gt: the incoming gradient tensor, true gradient = gs * Gt; gB = dT, the RRDB skip, which
// block 0 adds.  Channels [0,C) of dbuf(r) leave as the gradient with respect to the block's input
static int gen_bwd_block(GenBwd& c, int r, AfiView Gt, float gs, AfiView gB) {
    const GenPlan& p = c.p;
    const afi_gen_params_t *prm = c.prm, *gr = c.gr;
    const int N = c.N, H = c.H, W = c.W, C = prm->C, G = prm->G, L = (int)p.ws.L;
    const float rs = prm->residual_scale;
    AfiView b = c.buf(r), d = c.dbuf(r);
    const bool want_growth = gr->rdb_w[r][0] || gr->rdb_w[r][1] || gr->rdb_w[r][2] || gr->rdb_w[r][3];
    float* const packed = c.scratch + p.bws.o_rdbw + (long long)r * p.bws.n_rdbw;     // [4G][3][3][L]: pack_growth / batch_growth
    // conv5: out = x + rs*conv5(cat)
    c.fk.after_main();                                                     // Gt is complete
    if (gr->rdb_w[r][4]) AFI_TRY(c.wgrad(Gt, b, H, W, C, L, gr->rdb_w[r][4], rs * gs));
    {
        AfiPixGemm g = conv_dgrad_desc(Gt, N, H, W, C, prm->rdb_w[r][4], L, d);
        g.alpha = rs * gs;
        g.R1 = Gt; g.r1s = gs; g.r1_lo = 0; g.r1_hi = C;               // identity path of the block
        g.Z = b; g.z_lo = C + 3 * G; g.z_hi = L;                       // conv4's LReLU: its slice is final after this kernel
        c.im.attach(g, prm->rdb_w[r][4]);
        AFI_TRY(c.PG(g, 1));
    }
    for (int k = 4; k >= 1; --k) {
        const int cin = C + (k - 1) * G;
        AfiView dyk = ch_off(d, cin);                                   // d(pre-activation of conv_k), G channels
        c.fk.after_main();                                                 // dyk's slice was finalised by the previous dgrad
        if (gr->rdb_w[r][k - 1] && !p.bwd.batch_growth && !p.bwd.pack_growth) {
            const AfiWgradGemm wd = conv_wgrad_desc(dyk, b, N, H, W, G, cin, gr->rdb_w[r][k - 1], 1.f);
            AFI_TRY(p.bwd.grouped ? c.df.defer(c.cx, wd, c.st) : wgrad_launch(c.cx, wd, c.fk.side));
        }
        if (p.bwd.batch_growth) {
            // only the part of conv_k's data gradient that lands on y_1 .. y_{k-1} (channels [C, cin): (k-1) G columns) runs here, in chain
            // order -- each finalises the slice the next one reads; the parts that land on the block input x (channels [0, C)) of all four
            // convs are ONE data gradient from the 4G adjacent channels dy_1 .. dy_4 after the chain (below)
            if (k == 1) continue;
            AfiPixGemm g = conv_dgrad_desc(dyk, N, H, W, G, prm->rdb_w[r][k - 1] + C, cin - C, ch_off(d, C));
            g.b_sRow = 9LL * cin; g.b_sTap = cin;                       // (a column range of the [G][3][3][cin] weight)
            g.beta = 1.f;
            g.Z = ch_off(b, C); g.z_lo = cin - C - G; g.z_hi = cin - C;          // conv_{k-1}'s slice becomes final
            AFI_TRY(c.PG(g, 1));
            continue;
        }
        AfiPixGemm g = conv_dgrad_desc(dyk, N, H, W, G, prm->rdb_w[r][k - 1], cin, d);
        g.beta = 1.f;                                                   // dense connections: accumulate
        if (k >= 2) { g.Z = b; g.z_lo = cin - G; g.z_hi = cin; }        // conv_{k-1}'s slice becomes final
        if (k == 1 && r == 0) {                                         // RRDB skip (+dT) and the head conv's LReLU
            g.R2 = gB; g.r2s = 1.f; g.r2_lo = 0; g.r2_hi = C;
            g.Z = b; g.z_lo = 0; g.z_hi = C;
        }
        c.im.attach(g, prm->rdb_w[r][k - 1]);
        AFI_TRY(c.PG(g, 1));
    }
    // (every slice of d[C : C + 4G] is final now; each conv reads a prefix of b: rows of the packed gradient paired with channels behind their
    //  conv's input are computed and never read by the unpack)
    if (p.bwd.pack_growth && want_growth) {
        AFI_TRY(c.df.defer(c.cx, conv_wgrad_desc(ch_off(d, C), b, N, H, W, 4 * G, L, packed, 1.f), c.st));
        c.df.packed_mask |= 1u << r;
    }
    if (p.bwd.batch_growth) {
        // d[0:C) += sum_k W_k[:, :, :, 0:C]^T (*) dy_k: a 4G -> C data gradient on the packed weights [4G][3][3][C] -- Winograd-eligible at the
        // reference's widths (128 -> 256 channels) where the four per-conv ones (32 -> 256 .. 352) were direct GEMMs 288 deep
        const float* const wk[4] = {prm->rdb_w[r][0], prm->rdb_w[r][1], prm->rdb_w[r][2], prm->rdb_w[r][3]};
        float* Wx = c.scratch + p.bws.o_rdbx + (long long)r * p.bws.n_rdbx;
        bool hit = false, scratch_b = true;
        if (float* slot = wino_wcache_slot(c.cx, prm->rdb_w[r][0], /*tag: growth x-part pack*/ 3, 0, 4 * G, C, p.bws.n_rdbx, hit)) { Wx = slot; scratch_b = false; }
        if (!hit) AFI_TRY(afi_launch_rdb_xpart_pack(wk, Wx, C, G, c.st));
        AfiPixGemm g = conv_dgrad_desc(ch_off(d, C), N, H, W, 4 * G, Wx, C, d);
        g.beta = 1.f;
        g.no_wcache = scratch_b ? 1 : 0;
        if (r == 0) {                                                   // RRDB skip (+dT) and the head conv's LReLU
            g.R2 = gB; g.r2s = 1.f; g.r2_lo = 0; g.r2_hi = C;
            g.Z = b; g.z_lo = 0; g.z_hi = C;
        }
        AFI_TRY(c.PG(g, 1));
    }
    if (p.bwd.batch_growth && want_growth) {
        // the four growth convs' weight gradients as ONE product dy[C : C + 4G] (x) cat[0 : L]: a 4G-row GEMM -- Winograd F(3x3,4x4) on the bf16
        // matrix cores when 4G and L reach 128 channels -- instead of four G-row ones on the 32 x 128 fp32 tile, 1.26x their products at several
        // times their rate
        c.fk.after_main();
        hipStream_t sd = c.fk.side;
        if (hipMemsetAsync(packed, 0, sizeof(float) * 4LL * G * 9 * L, sd) != hipSuccess) return AFI_ERR_LAUNCH;
        const AfiView dy4 = ch_off(d, C);
        WinoWgradOpt o;
        o.accumulate = false;
        if (gen_wino_wgrad_ok(c.cx, p, 4 * G, L, p.ws.P, wino_ws_floats(N, H, W, L, 4 * G)))
            AFI_TRY(wino_wgrad(c.cx, dy4, b, N, H, W, 4 * G, L, packed, 1.f, c.scratch + p.bws.o_wino2, p.bws.n_wino, sd, o));
        else AFI_TRY(wgrad_launch(c.cx, conv_wgrad_desc(dy4, b, N, H, W, 4 * G, L, packed, 1.f), sd));
        float* const dws[4] = {gr->rdb_w[r][0], gr->rdb_w[r][1], gr->rdb_w[r][2], gr->rdb_w[r][3]};
        AFI_TRY(afi_launch_rdb_wgrad_unpack(packed, dws, C, G, 1.f, sd));
    }
    return AFI_OK;
}

int afi_generator_bwd(afi_ctx_t* cx, const afi_gen_params_t* prm, const afi_gen_params_t* gr, afi_view_t xv, int N, int H, int W, const float* ws,
                      const float* dout, float* dx, float* scratch, long long scratch_floats, void* stream) {
    AFI_CTX_CHECK(cx);
    AFI_TRY(gen_check(prm));
    if (!gr || N <= 0 || H <= 0 || W <= 0 || !ws || !dout || !scratch) return AFI_ERR_BAD_ARG;
    const int C = prm->C, R = prm->n_rdb;
    const GenPlan p = gen_plan(cx, C, prm->G, R, N, H, W);
    const GenWs& l = p.ws;
    const GenBwdWs& s = p.bws;
    if (scratch_floats < s.total) return AFI_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    GenBwd c(cx, p, prm, gr, N, H, W, ws, scratch, st);
    const int L = (int)l.L;
    const long long P = l.P;
    AfiView x = V(xv);
    AfiView t = dense_view(ws + l.o_t, H, W, C), a7 = dense_view(ws + l.o_a7, H, W, C);
    AfiView u = dense_view(ws + l.o_u, 2 * H, 2 * W, C);
    AfiView dOut = dense_view(dout, 2 * H, 2 * W, C);
    AfiView dU = dense_view(scratch + s.o_du, 2 * H, 2 * W, C);
    AfiView gA = dense_view(scratch + s.o_ga, H, W, C), gB = dense_view(scratch + s.o_gb, H, W, C);
    float* dwp = scratch + s.o_dwp;                        // the conv-transpose gradient in packed form
    // zero fill of the packed gradients the grouped launches add into: dwp and the blocks' packed growth gradients in one piece where they are
    // neighbours (Bwd::one_fill) and dwp is wanted, else the growth gradients here and dwp at its use
    const bool one_fill = p.bwd.one_fill && gr->wT;
    const long long n_dwp = align4(36LL * C * C), n_fill = (one_fill ? n_dwp : 0) + (long long)R * s.n_rdbw;
    float* const fill = scratch + s.o_rdbw - (one_fill ? n_dwp : 0);
    bool filled = false, skip_grad_done = false;
    if (p.bwd.images) {
        Wk6Req rq[kWk6MaxReq];
        // riders of the image launch (they depend on nothing this pass computes): that zero fill and the skip path's gradient into dx
        AfiWk6Side side;
        memset(&side, 0, sizeof(side));
        if (one_fill && (((uintptr_t)fill) & 15) == 0) { side.zero_p = fill; side.zero_n4 = n_fill / 4; }
        if (dx && (C & 3) == 0) { side.bl_dout = dout; side.bl_dx = dx; side.bl_N = N; side.bl_H = H; side.bl_W = W; side.bl_C = C; }
        bool rode = false;
        AFI_TRY(wk6_build(cx, c.im, rq, gen_bwd_image_reqs(p, prm, dx != nullptr, rq), scratch + s.o_img, s.n_img, st, &side, &rode));
        filled = rode && side.zero_p;
        skip_grad_done = rode && side.bl_dx;
    }
    if (p.bwd.pack_growth && !filled && hipMemsetAsync(fill, 0, sizeof(float) * (size_t)n_fill, st) != hipSuccess) return AFI_ERR_LAUNCH;
    {   // the flipped f16x3 weight images of the pass's Winograd data gradients that the cache does not hold yet, in one builder call on the main
        // stream (the side stream runs weight gradients only: they read no weight image): the data gradients below, in their order, by the
        // fields wino_eligible and wino_form read.  The growth convs' packed x-part takes its cache slot (and is packed) where the walk meets it
        WinoImgBatch ib(cx);
        const int G = prm->G;
        auto want = [&](AfiPixGemm g, const float* key) { if (key) c.im.attach(g, key); ib.add(g, 1, s.n_wino, false); };
        want(conv_dgrad_desc(dOut, N, 2 * H, 2 * W, C, prm->w9, C, dU), prm->w9);
        want(convT_dgrad_desc(dU, N, H, W, C, ws + l.o_wp, C, gA), prm->wT);
        want(conv_dgrad_desc(gA, N, H, W, C, prm->w7, C, gB), prm->w7);
        for (int r = R - 1; r >= 0 && ib.open; --r) {
            want(conv_dgrad_desc(gB, N, H, W, C, prm->rdb_w[r][4], L, c.dbuf(r)), prm->rdb_w[r][4]);
            if (p.bwd.batch_growth) {
                // (the chain's partial data gradients read G < 128 channels: never in Winograd form)
                const float* const wk[4] = {prm->rdb_w[r][0], prm->rdb_w[r][1], prm->rdb_w[r][2], prm->rdb_w[r][3]};
                bool hit = false;
                if (float* slot = wino_wcache_slot(cx, prm->rdb_w[r][0], /*tag: growth x-part pack*/ 3, 0, 4 * G, C, s.n_rdbx, hit)) {
                    if (!hit) AFI_TRY(afi_launch_rdb_xpart_pack(wk, slot, C, G, st));
                    want(conv_dgrad_desc(c.dbuf(r), N, H, W, 4 * G, slot, C, c.dbuf(r)), nullptr);
                }
            } else {
                for (int k = 4; k >= 1; --k) want(conv_dgrad_desc(c.dbuf(r), N, H, W, G, prm->rdb_w[r][k - 1], C + (k - 1) * G, c.dbuf(r)), prm->rdb_w[r][k - 1]);
            }
        }
        if (dx) want(conv_dgrad_desc(gB, N, H, W, C, prm->w0, C, dense_view(dx, H, W, C)), prm->w0);
        AFI_TRY(ib.build(scratch + s.o_wino, st));
    }

    // ---- final conv (generator_rdb.py:107-108)
    if (gr->w9) AFI_TRY(c.wgrad(dOut, u, 2 * H, 2 * W, C, C, gr->w9, 1.f));
    if (gr->b9) AFI_TRY(c.colsum(dout, 4 * P, C, C, gr->b9));
    {
        AfiPixGemm g = conv_dgrad_desc(dOut, N, 2 * H, 2 * W, C, prm->w9, C, dU);
        g.Z = u; g.z_lo = 0; g.z_hi = C;                       // through the LReLU after the conv-transpose
        c.im.attach(g, prm->w9);                               // (GenPlan::hires_wk6: the small-map kernel instead of the five Winograd launches)
        AFI_TRY(c.PG(g, 1));
    }
    // ---- conv-transpose (:101-105)
    c.fk.after_main();                                                      // dU is complete
    if (gr->wT) {
        hipStream_t sd = c.fk.side;
        if (!one_fill && hipMemsetAsync(dwp, 0, sizeof(float) * 36LL * C * C, sd) != hipSuccess) return AFI_ERR_LAUNCH;
        if (p.bwd.grouped) {
            AFI_TRY(c.df.defer(cx, convT_wgrad_desc(dU, a7, N, H, W, C, C, dwp, 1.f), st));
            c.df.convT = true;
        } else if (gen_wino_wgrad_ok(cx, p, 4 * C, C, P)) {              // the four phases as channel blocks of one Winograd weight gradient
            WinoWgradOpt o;
            o.dy_phases = 4; o.accumulate = false;
            AFI_TRY(wino_wgrad(cx, dU, a7, N, H, W, 4 * C, C, dwp, 1.f, scratch + s.o_wino2, s.n_wino, sd, o));
        } else {
            AFI_TRY(wgrad_launch(cx, convT_wgrad_desc(dU, a7, N, H, W, C, C, dwp, 1.f), sd));
        }
        if (!p.bwd.grouped) AFI_TRY(afi_launch_convT_unpack_grad(dwp, gr->wT, C, C, sd));
    }
    if (gr->bT) AFI_TRY(c.colsum(dU.p, 4 * P, C, C, gr->bT));
    {
        AfiPixGemm g = convT_dgrad_desc(dU, N, H, W, C, ws + l.o_wp, C, gA);
        g.Z = a7; g.z_lo = 0; g.z_hi = C;
        c.im.attach(g, prm->wT);
        AFI_TRY(c.PG(g, 1));
    }
    // ---- trunk conv (:97-99): gA = d(pre-activation of a7)
    c.fk.after_main();                                                      // gA is complete
    if (gr->w7) AFI_TRY(c.wgrad(gA, t, H, W, C, C, gr->w7, 1.f));
    if (gr->b7) AFI_TRY(c.colsum(gA.p, P, C, C, gr->b7));
    {
        AfiPixGemm g = conv_dgrad_desc(gA, N, H, W, C, prm->w7, C, gB);  // gB = dT
        c.im.attach(g, prm->w7);
        AFI_TRY(c.PG(g, 1));
    }
    // ---- ResidualInResidual (:27-30) and the RDB chain (:64-71), last block first
    AfiView Gt = gB;
    for (int r = R - 1; r >= 0; --r) {
        AFI_TRY(gen_bwd_block(c, r, Gt, r == R - 1 ? prm->residual_scale : 1.f, gB));
        Gt = c.dbuf(r);
    }
    // ---- head conv (:91-93): Gt[0:C] = d(pre-activation of a0)
    c.fk.after_main();
    if (gr->w0) AFI_TRY(c.wgrad(Gt, x, H, W, C, C, gr->w0, 1.f));
    if (gr->b0) AFI_TRY(c.colsum(Gt.p, P, C, L, gr->b0));
    if (dx) {
        if (!skip_grad_done) AFI_TRY(afi_launch_bilinear2x_bwd(dout, N, H, W, C, 0.f, dx, st));           // skip path (:125)
        AfiPixGemm g = conv_dgrad_desc(Gt, N, H, W, C, prm->w0, C, dense_view(dx, H, W, C));
        g.beta = 1.f;
        c.im.attach(g, prm->w0);
        AFI_TRY(c.PG(g, 1));
    }
    AFI_TRY(c.df.flush(p, prm, gr, scratch, st));          // everything a grouped pass deferred
    c.fk.join();
    return AFI_OK;
}

// ------------------------------------------------------------------------------------------------ discriminator
// forward workspace (floats): [c0 P*F1][y0 P*F1][c1 P*F2][y1 P*F2][c2 P*F3][d9 P*16][mean,invstd x3][red] ... [y2 P*F3, where it is written][kept planes]
struct DiscWs {
    long long P;
    long long o_c[3], o_y[3], o_d9, o_mean[3], o_invstd[3], o_red, o_stats, o_amax, o_part, n_part, o_wino, n_wino, o_mean_b[3], o_invstd_b[3], o_vkeep[3], total;
};
// keep_mask: bit n reserves the kept F(4x4) input planes of block n (DiscPlan::Block::keep).  The planes sit at the END of the layout, so every other
// offset is the same under every mask; the context-free queries reserve them wherever some context could keep them (disc_ws_bound), the
// context-aware one (afi_discriminator_fwd_ws_floats_ex) and the two passes where the plan keeps them (an fp32 / bf16x6 context, a
// forward no backward follows and the F(2x2) blocks paid 0.6 + 1.25 GB per workspace at P2 for planes nobody writes)
// y2: reserve the last block's activation (P x F3 floats, the largest tensor of the network): not under AFI_OPT_D_FUSE_TAIL, where nobody writes
// it.  It sits behind every fixed region (its offset is the same either way: afi_discriminator_ws_layout is context-free) and in front of the kept planes.
static DiscWs disc_ws(const int F[4], int N, int H, int W, int keep_mask, bool y2) {
    DiscWs w;
    w.P = (long long)N * H * W;
    long long o = 0;
    int fmax = 4;
    for (int n = 0; n < 3; ++n) {
        w.o_c[n] = o; o += align4(w.P * F[n + 1]);
        if (n < 2) { w.o_y[n] = o; o += align4(w.P * F[n + 1]); }
        if (F[n + 1] > fmax) fmax = F[n + 1];
    }
    w.o_d9 = o; o += align4(w.P * 16);
    for (int n = 0; n < 3; ++n) {
        w.o_mean[n] = o; o += align4(F[n + 1]);
        w.o_invstd[n] = o; o += align4(F[n + 1]);
    }
    w.o_red = o; o += align4(afi_reduce_scratch_floats(fmax));
    w.o_stats = o; o += 4LL * AFI_STATS_MAX_ROWS * fmax;  // fp64 partial rows [rows][2][C] of the statistics fused into the output transforms
    w.o_amax = o; o += 16;                                // [4 n]: the largest magnitude of block n's INPUT (x, y0, y1), raised by its producer (Winograd path; kept for the backward)
    w.n_part = part_floats({w.P * F[1], w.P * F[2], w.P * F[3]});
    w.o_part = o; o += w.n_part;
    w.n_wino = disc_wino_floats(F, N, H, W);              // transient: Winograd U / V / M buffers, shared by the three convs
    w.o_wino = o; o += w.n_wino;
    for (int n = 0; n < 3; ++n) {                         // the second half's batch statistics of a paired call (afi_discriminator_fwd_paired)
        w.o_mean_b[n] = o; o += align4(F[n + 1]);
        w.o_invstd_b[n] = o; o += align4(F[n + 1]);
    }
    w.o_y[2] = o;
    if (y2) o += align4(w.P * F[3]);
    for (int n = 0; n < 3; ++n) {
        w.o_vkeep[n] = o;
        if ((keep_mask >> n) & 1) o += align4(36 * wino4_tpad(N, H, W) * F[n]);
    }
    w.total = o;
    return w;
}
// blocks 1 and 2 (the only ones that keep planes) wherever their form can be F(4x4), and y2
static DiscWs disc_ws_bound(const int F[4], int N, int H, int W) { return disc_ws(F, N, H, W, (long long)N * H * W >= kWinoF4MinPixels ? 6 : 0, true); }
struct DiscBwdWs { long long o_g[3], o_dd9, o_amax, o_red, o_red2, o_tail, o_part, n_part, o_wino, n_wino, o_wino2, total; };
static DiscBwdWs disc_bwd_ws(const int F[4], int N, int H, int W) {
    DiscBwdWs w;
    const long long P = (long long)N * H * W;
    int fmax = 4;
    for (int n = 0; n < 4; ++n) if (F[n] > fmax) fmax = F[n];
    long long o = 0;
    for (int n = 0; n < 3; ++n) { w.o_g[n] = o; o += align4(P * F[n + 1]); }   // one gradient buffer per block (no ping-pong reuse)
    w.o_dd9 = o; o += align4(P * 16);
    w.o_amax = o; o += 16;                                // [4 n]: the largest magnitude of d(conv output of block n), raised by the BatchNorm backward (Winograd path)
    w.o_red = o; o += align4(afi_reduce_scratch_floats(fmax));       // BatchNorm backward (main stream)
    w.o_red2 = o; o += align4(afi_reduce_scratch_floats(fmax));      // bias column sums (side stream)
    w.o_tail = o; o += align4(afi_disc_tail_scratch_floats(F[3]));   // the fused tail's partial sums (AFI_OPT_D_FUSE_TAIL)
    w.n_part = part_floats({P * F[0], P * F[1], P * F[2], P * F[3]});
    w.o_part = o; o += w.n_part;
    w.n_wino = disc_wino_floats(F, N, H, W);
    w.o_wino = o; o += w.n_wino;                          // data-gradient chain (main stream)
    w.o_wino2 = o; o += w.n_wino;                         // weight gradients (they may run on the side stream beside it)
    w.total = o;
    return w;
}

// Everything a discriminator call decides.  A forward (training as afi_discriminator_fwd's) and the backward that follows it (training == 1) build
// their plan from the same context, shape and pairing, which is why afi_discriminator_bwd must run under the options and the arithmetic of its
// forward: the backward reads the layout and the kept planes this plan says the forward wrote.
struct DiscPlan {
    // the three 3x3 convs in Winograd form: from ~1 K pixels on the 2.25x fewer matrix-core FLOPs win over the transform traffic (measured:
    // 2x336x200 1024->1024 18.8 -> 11.8 ms, 2x84x50 1.38 -> 0.72 ms).  AFI_OPT_WINOGRAD = 0 switches it off, AFI_OPT_D_WINOGRAD_MIN_PIXELS moves
    // the threshold (not below the 1024 pixels the workspace queries size the scratch from)
    bool wino;
    // AFI_OPT_D_FUSE_TAIL in force for F3 last-block channels: block 2's apply pass, the last conv and their backward run as the fused passes of
    // csrc/elementwise.hip (afi_launch_disc_tail_*): y[2] and the gradient with respect to it are never written
    bool tail;
    // the forward leaves every block input's largest magnitude in DiscWs::o_amax, whatever arithmetic it runs in (the backward trusts the slots):
    // x's by the first input transform; y0's / y1's by the BatchNorm apply passes
    bool fwd_amax;
    // the backward (f16x3) raises the largest magnitude of every d(conv output) into DiscBwdWs::o_amax, by the BatchNorm backward that writes it:
    // with the forward's slots every Winograd transform of the pass knows its source's maximum beforehand and writes its planes pre-split
    bool bwd_amax;
    // x comes from outside the library: where block 0's GEMM is to take the k-step-local sums its maximum is measured first, one streaming pass
    // over x (137 MB, ~30 us at 2x200x336).  This test asks less than block 0's form (F[0] % 32 == 0 but not WinoForm::presplit's F[1] % 128):
    // it is the one that governs, so at F0 = 32 x is measured although block 0's planes are not written pre-split
    bool x_amax;
    struct Block {
        WinoForm fwd, wgrad;   // the forms of the block's forward conv and of its weight gradient
        bool local_sums;       // AFI_OPT_F16_LOCAL_SUMS: the forward's GEMM takes k-step-local sums
        bool stats;            // the forward's output transform accumulates the BatchNorm statistics (training, one affine per tensor, shapes it takes)
        // the forward keeps its input planes for the backward's weight gradient: both forms keep, and the input's maximum is known before its
        // transform runs (blocks 1 and 2).  The weight gradient's channel test governs: F[n] % 128 == 0, where the forward's form asks
        // F[n] % 32 == 0 (at F0 = 32 block 1 keeps nothing)
        bool keep;
    } b[3];
    DiscWs ws;        // the forward's layout: planes reserved where a plain OR a paired call of this training mode keeps them
    DiscBwdWs bws;
};
static DiscPlan disc_plan(const afi_ctx* cx, const int F[4], int N, int H, int W, int training, int halves) {
    DiscPlan p;
    const long long minpix = afi_opt(cx, AFI_OPT_D_WINOGRAD_MIN_PIXELS);
    p.wino = disc_wino_floats(F, N, H, W) > 0 && afi_opt(cx, AFI_OPT_WINOGRAD) && (long long)N * H * W >= (minpix < 1024 ? 1024 : minpix);
    p.tail = afi_opt(cx, AFI_OPT_D_FUSE_TAIL) != 0 && !(F[3] & 15) && F[3] <= 1024;
    const int dtype = cx ? cx->dtype : afi_default_dtype();
    p.fwd_amax = p.wino;
    p.bwd_amax = p.wino && dtype == AFI_DTYPE_F16X3;
    p.x_amax = p.wino && training == 1 && disc_local_sums(cx, 0) && dtype == AFI_DTYPE_F16X3 && afi_opt(cx, AFI_OPT_F16_PRESPLIT) != 0 && !(F[0] & 31);
    int keep_mask = 0;
    for (int n = 0; n < 3; ++n) {
        DiscPlan::Block& b = p.b[n];
        b.fwd = wino_form(cx, N, H, W, F[n], F[n + 1], training != 1 || wino_d_f4(cx, n) ? kWinoFwdF4 : kWinoFwd);
        b.wgrad = wino_form(cx, N, H, W, F[n], F[n + 1], kWinoWgrad);
        b.local_sums = training == 1 && disc_local_sums(cx, n);
        b.stats = p.wino && training && halves == 1 && afi_opt(cx, AFI_OPT_BN_STATS_FP64) != 0 && afi_wino_stats_rows(b.fwd.T, F[n + 1]) > 0;
        b.keep = n > 0 && training == 1 && p.wino && b.fwd.keep && b.wgrad.keep;
        if (b.keep) keep_mask |= 1 << n;
    }
    p.ws = disc_ws(F, N, H, W, keep_mask, !p.tail);
    p.bws = disc_bwd_ws(F, N, H, W);
    return p;
}

long long afi_discriminator_fwd_ws_floats(const int F[4], int N, int H, int W) { return disc_ws_bound(F, N, H, W).total; }
long long afi_discriminator_fwd_ws_floats_ex(const afi_ctx_t* ctx, const int F[4], int N, int H, int W, int training) {
    if (!F || N <= 0 || H <= 0 || W <= 0) return 0;
    return disc_plan(ctx, F, N, H, W, training, 1).ws.total;     // (plain or paired call)
}
// where the forward keeps what the backward reads (offsets in floats into the forward workspace, the same in every plan's layout): 12 entries,
// conv outputs c[0..2] ([P][F_{n+1}]), activations y[0..2], batch means [F_{n+1}], 1/sqrt(var + eps) [F_{n+1}]
int afi_discriminator_ws_layout(const int F[4], int N, int H, int W, long long* off12) {
    if (!F || !off12 || N <= 0 || H <= 0 || W <= 0) return AFI_ERR_BAD_ARG;
    const DiscWs l = disc_ws_bound(F, N, H, W);
    for (int n = 0; n < 3; ++n) { off12[n] = l.o_c[n]; off12[3 + n] = l.o_y[n]; off12[6 + n] = l.o_mean[n]; off12[9 + n] = l.o_invstd[n]; }
    return AFI_OK;
}
int afi_discriminator_saved_activations(const afi_ctx_t* ctx, const int F[4], int N, int H, int W) {
    if (!F || N <= 0 || H <= 0 || W <= 0) return -1;
    const DiscPlan p = disc_plan(ctx, F, N, H, W, 1, 1);
    return 3 | (p.tail ? 0 : 4);                           // (y[2]: read by the last conv only)
}
long long afi_discriminator_bwd_ws_floats(const int F[4], int N, int H, int W) { return disc_bwd_ws(F, N, H, W).total; }

static int disc_check(const afi_disc_params_t* p) {
    if (!p) return AFI_ERR_BAD_ARG;
    for (int n = 0; n < 4; ++n) {
        if (p->F[n] <= 0) return AFI_ERR_BAD_ARG;
        if (p->F[n] & 3) return AFI_ERR_UNSUPPORTED;
    }
    return AFI_OK;
}

}  // extern "C"

// `halves` = 1: the reference's call.  `halves` = 2 (afi_discriminator_fwd_paired): images [0, N/2) and [N/2, N) are two calls of the reference made one
// after the other (D(real) then D(fake) in the D phase, stage1_trainer.py:349-359; D(fake) then D(real) in the G phase, :399-403) -- every conv
// runs once over all N images, every BatchNorm takes its batch statistics per half and moves the running statistics twice, first half first.
static int disc_fwd(afi_ctx_t* ctx, const afi_disc_params_t* prm, afi_view_t xv, int N, int H, int W, int halves, float* logits, int training, float* ws,
                    long long ws_floats, void* stream) {
    afi_ctx* cx = ctx; (void)cx;
    AFI_CTX_CHECK(ctx);
    AFI_TRY(disc_check(prm));
    const bool stats_only = training == 3;                 // BatchNorm side effects only: no last activation, last conv or logits
    if (N <= 0 || H <= 0 || W <= 0 || !ws || !xv.p || (!logits && !stats_only)) return AFI_ERR_BAD_ARG;
    if ((halves != 1 && halves != 2) || N % halves) return AFI_ERR_BAD_ARG;
    const DiscPlan pl = disc_plan(cx, prm->F, N, H, W, training, halves);
    const DiscWs& l = pl.ws;                               // (the layout afi_discriminator_fwd_ws_floats_ex sizes)
    if (ws_floats < l.total) return AFI_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    float* const part_ = ws + l.o_part;
    const long long part_n_ = l.n_part;
    auto PG = [&](AfiPixGemm g, int b_rc) { g.partial = part_; g.partial_floats = part_n_; return afi_launch_pix_gemm(g, b_rc, st); };
    const long long P = l.P;
    float* red = ws + l.o_red;
    AfiView in = V(xv);
    const bool wino = pl.wino, tail = pl.tail;
    const long long Ph = P / halves;
    float* amax = ws + l.o_amax;                            // (DiscPlan::fwd_amax)
    if (pl.fwd_amax && hipMemsetAsync(amax, 0, 16 * sizeof(float), st) != hipSuccess) return AFI_ERR_LAUNCH;
    if (wino) {                                             // the three forward weight images the cache does not hold yet, in one builder call
        WinoImgBatch ib(cx);
        for (int n = 0; n < 3; ++n) ib.add(prm->w[n], prm->F[n], prm->F[n + 1], pl.b[n].fwd);
        AFI_TRY(ib.build(ws + l.o_wino, st));
    }
    bool in_known = false;                                  // block n's input maximum is published before its transform runs
    if (pl.x_amax) {
        AFI_TRY(afi_launch_view_absmax(in, N, H, W, prm->F[0], amax, st));
        in_known = true;
    }
    for (int n = 0; n < 3; ++n) {       // Conv2d 3x3 + bias -> BN -> LeakyReLU (feature_patch_discriminator.py:35-38)
        const int ci = prm->F[n], co = prm->F[n + 1];
        float* c = ws + l.o_c[n]; float* y = ws + l.o_y[n];
        float* mean = ws + l.o_mean[n]; float* invstd = ws + l.o_invstd[n];
        const DiscPlan::Block& b = pl.b[n];
        int stats_rows = 0;
        double* stats = (double*)(ws + l.o_stats);          // (8-byte aligned: every offset of the layout is a multiple of 4 floats and ws comes from an allocator)
        const bool fuse_stats = b.stats && (((uintptr_t)stats) & 7) == 0;
        if (wino) {
            if (b.keep && !in_known) return AFI_ERR_LAUNCH; // (the plan promised a known maximum: never hand the backward planes this pass cannot split)
            WinoConvOpt o;
            if (fuse_stats) { o.stats = stats; o.stats_rows = &stats_rows; }
            o.in_amax = pl.fwd_amax ? amax + 4 * n : nullptr; o.in_amax_known = in_known;
            o.v_keep = b.keep ? ws + l.o_vkeep[n] : nullptr; o.local_sums = b.local_sums;
            AFI_TRY(wino_conv(cx, b.fwd.kind, in, N, H, W, ci, prm->w[n], co, prm->b[n], dense_view(c, H, W, co), null_view(), ws + l.o_wino, l.n_wino, part_,
                              part_n_, st, o));
        } else {
            AFI_TRY(PG(conv_fwd_desc(in, N, H, W, ci, prm->w[n], prm->b[n], co, dense_view(c, H, W, co)), 0));
        }
        // nothing reads the last block's activation / the last conv reads c through the affine
        const bool skip_apply = (stats_only && n == 2) || (n == 2 && tail);
        const float* mean_used = mean;
        if (!training) {
            AFI_TRY(afi_launch_invstd(prm->running_var[n], invstd, co, st));
            mean_used = prm->running_mean[n];
        }
        in_known = false;
        for (int h = 0; h < halves; ++h) {
            float* mean_h = h ? ws + l.o_mean_b[n] : mean;
            float* invstd_h = h ? ws + l.o_invstd_b[n] : invstd;
            const float* ch = c + (long long)h * Ph * co;
            if (training && stats_rows > 0) {               // the output transform accumulated the sums while it stored c: only the finalizer is left
                AFI_TRY(afi_launch_bn_stats_from_partials(stats, stats_rows, P, co, mean, invstd, nullptr, prm->running_mean[n], prm->running_var[n], st,
                                                          prm->num_batches_tracked[n]));
            } else if (training) {
                AFI_TRY(afi_launch_bn_stats(ch, Ph, co, mean_h, invstd_h, nullptr, prm->running_mean[n], prm->running_var[n], red, st,
                                            prm->num_batches_tracked[n], -1.f, -1.f, afi_opt(cx, AFI_OPT_BN_STATS_FP64) != 0));  // the counter ticks inside the statistics finalizer
            }
            if (!skip_apply) {
                AFI_TRY(afi_launch_bn_apply_lrelu(ch, y + (long long)h * Ph * co, training ? mean_h : mean_used, training ? invstd_h : invstd, prm->gamma[n],
                                                  prm->beta[n], Ph, co, st, AFI_LRELU_SLOPE, pl.fwd_amax && n < 2 ? amax + 4 * (n + 1) : nullptr));
                in_known = pl.fwd_amax && n < 2;                 // (published by the pass that wrote the activation)
            }
        }
        in = dense_view(y, H, W, co);
    }
    if (!stats_only && tail) {   // last conv 3x3 F3 -> 1 (:40-41) reading c2 through block 2's affine + LeakyReLU (y2 is never written), then the 9-tap stencil
        const int F3 = prm->F[3];
        float* d9 = ws + l.o_d9;
        for (int h = 0; h < halves; ++h) {                  // (a paired call: each half through its own batch statistics)
            const AfiBnLoad bn{training ? (h ? ws + l.o_mean_b[2] : ws + l.o_mean[2]) : prm->running_mean[2], training && h ? ws + l.o_invstd_b[2] : ws + l.o_invstd[2],
                               prm->gamma[2], prm->beta[2]};
            AFI_TRY(afi_launch_disc_tail_fwd(ws + l.o_c[2] + (long long)h * Ph * F3, &bn, AFI_LRELU_SLOPE, prm->w3, d9 + (long long)h * Ph * 16, Ph, F3, st));
        }
        AFI_TRY(afi_launch_stencil9_sum(d9, 16, prm->b3, logits, N, H, W, st));
    } else if (!stats_only) {   // ... D9[q][t] = <y2[q], w3[t]> on the MFMA kernel (1x1, 9 columns)
        const int F3 = prm->F[3];
        float* d9 = ws + l.o_d9;
        AfiPixGemm g = pix_default(N, H, W);
        g.ntaps = 1; g.Ck = F3; g.Ncols = 9; g.CoutPhase = 9;
        g.A = in; g.B = prm->w3; g.b_sRow = F3; g.b_sTap = 0;
        g.O = dense_view(d9, H, W, 16);
        AFI_TRY(PG(g, 0));
        AFI_TRY(afi_launch_stencil9_sum(d9, 16, prm->b3, logits, N, H, W, st));
    }
    return AFI_OK;
}

static int disc_bwd(afi_ctx_t* ctx, const afi_disc_params_t* prm, const afi_disc_params_t* gr, afi_view_t xv, int N, int H, int W, int halves, const float* ws,
                    const float* dlogits, float* dx, float* scratch, long long scratch_floats, void* stream) {
    afi_ctx* cx = ctx; (void)cx;
    AFI_CTX_CHECK(ctx);
    AFI_TRY(disc_check(prm));
    if (!gr || N <= 0 || H <= 0 || W <= 0 || !ws || !dlogits || !scratch) return AFI_ERR_BAD_ARG;
    if ((halves != 1 && halves != 2) || N % halves) return AFI_ERR_BAD_ARG;
    const DiscPlan pl = disc_plan(cx, prm->F, N, H, W, 1, halves);
    const DiscWs& l = pl.ws;                               // the layout its forward (training == 1, same context settings) wrote
    const DiscBwdWs& s = pl.bws;
    if (scratch_floats < s.total) return AFI_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    float* const part_ = scratch + s.o_part;
    const long long part_n_ = s.n_part;
    auto PG = [&](AfiPixGemm g, int b_rc) { g.partial = part_; g.partial_floats = part_n_; return afi_launch_pix_gemm(g, b_rc, st); };
    const long long P = l.P;
    float* red = scratch + s.o_red;
    float* red2 = scratch + s.o_red2;
    float* dd9 = scratch + s.o_dd9;
    if (pl.wino) {                                          // the flipped weight images of the pass's data gradients, last block first, before the side stream forks
        WinoImgBatch ib(cx);
        for (int n = 2; n >= (dx ? 0 : 1); --n) ib.add(prm->w[n], prm->F[n + 1], prm->F[n], wino_form(cx, N, H, W, prm->F[n + 1], prm->F[n], kWinoDgrad));
        AFI_TRY(ib.build(scratch + s.o_wino, st));
    }
    // (round 3, re-measured with the DMA GEMM: forking the weight gradients of LARGE maps onto the side stream too: 113.2 vs 112.5 ms per step,
    //  two A/B pairs on one box -- the chip has no room left beside the GEMMs)
    Fork fk(cx, st, P <= kSideStreamMaxPixels);
    hipStream_t sd = fk.side;                              // weight / bias gradients run beside the data-gradient chain
    const bool wino = pl.wino, tail = pl.tail;
    const int F3 = prm->F[3];
    float* gmax = scratch + s.o_amax;                      // (DiscPlan::bwd_amax; the forward filled its slots, xmax)
    const bool bwd_amax = pl.bwd_amax;
    if (bwd_amax && hipMemsetAsync(gmax, 0, 16 * sizeof(float), st) != hipSuccess) return AFI_ERR_LAUNCH;
    const float* xmax = ws + l.o_amax;
    // ---- last conv
    if (gr->b3) AFI_TRY(afi_launch_sum_accum(dlogits, P, 1.f, gr->b3, sd));
    AFI_TRY(afi_launch_stencil9_scatter(dlogits, dd9, 16, N, H, W, st));
    fk.after_main();                                       // dd9 is complete
    // (under the fused tail the forward wrote no y2: its readers below are the fused passes)
    AfiView y2 = dense_view(ws + l.o_y[2], H, W, F3);
    if (gr->w3 && !tail) {
        AfiWgradGemm g = conv_wgrad_desc(dense_view(dd9, H, W, 16), y2, N, H, W, 9, F3, gr->w3, 1.f);
        g.ntaps = 1; g.dw_sRow = F3; g.dw_sTap = 0;
        AFI_TRY(wgrad_launch(cx, g, sd));
    }
    if (!tail) {
        AfiPixGemm g = pix_default(N, H, W);
        g.ntaps = 1; g.a_sgn = -1; g.Ck = 9; g.Ncols = F3; g.CoutPhase = F3;
        g.A = dense_view(dd9, H, W, 16); g.B = prm->w3; g.b_sRow = F3; g.b_sTap = 0;
        g.O = dense_view(scratch + s.o_g[2], H, W, F3);      // gradient w.r.t. the ACTIVATION y2: its LeakyReLU' mask is applied by the BN backward
        AFI_TRY(PG(g, 1));
    }
    // ---- conv + BN + LReLU blocks, last first
    for (int n = 2; n >= 0; --n) {
        const int ci = prm->F[n], co = prm->F[n + 1];
        float* g_ = scratch + s.o_g[n];               // d(activation of block n)
        const float* c = ws + l.o_c[n];
        // LeakyReLU' and BatchNorm backward in one: the mask is recomputed from the saved conv output (the same pinned affine the forward
        // evaluated: bit-identical decisions) inside the two passes that read it anyway, instead of streaming the activation through
        // the producing data gradient's output transform as a third operand
        for (int h = 0; h < halves; ++h) {            // (a paired call: each half against its own batch statistics; the parameter gradients add up)
            const long long Ph = P / halves, o = (long long)h * Ph * co;
            if (n == 2 && tail) {                     // the gradient w.r.t. y2 is generated from dd9, the last conv's weight gradient rides with the sums
                const AfiBnLoad bn{ws + (h ? l.o_mean_b[n] : l.o_mean[n]), ws + (h ? l.o_invstd_b[n] : l.o_invstd[n]), prm->gamma[n], prm->beta[n]};
                AFI_TRY(afi_launch_disc_tail_bwd(c + o, dd9 + (long long)h * Ph * 16, bn, AFI_LRELU_SLOPE, prm->w3, g_ + o, gr->gamma[n], gr->beta[n], gr->w3, Ph, co,
                                                 scratch + s.o_tail, bwd_amax ? gmax + 4 * n : nullptr, st));
                continue;
            }
            AFI_TRY(afi_launch_bn_bwd(g_ + o, c + o, g_ + o, ws + (h ? l.o_mean_b[n] : l.o_mean[n]), ws + (h ? l.o_invstd_b[n] : l.o_invstd[n]), prm->gamma[n],
                                      gr->gamma[n], gr->beta[n], 1.f, Ph, co, red, st, prm->beta[n], AFI_LRELU_SLOPE,
                                      bwd_amax ? gmax + 4 * n : nullptr));                                              // in place: g_ = d(conv output)
        }
        fk.after_main();                              // g_ = d(conv output) is complete
        // d(loss)/d(bias) of a conv that feeds a train-mode BatchNorm is EXACTLY zero: g_ = BN backward's dx, whose sum over the pixels
        // of a channel vanishes identically (the BN output does not change when a constant is added to its input).  The reference
        // accumulates the fp32 rounding noise of that sum (~1e-7 of |g|); adding nothing to gr->b[n] is the exact value and saves a
        // full HBM pass over g_ per layer.  (Eval-mode BN has no backward here; the bias of the last conv is handled above.)
        (void)red2;
        AfiView gy = dense_view(g_, H, W, co);
        AfiView xin = (n == 0) ? V(xv) : dense_view(ws + l.o_y[n - 1], H, W, ci);
        if (gr->w[n] && wino) {
            WinoWgradOpt o;
            if (bwd_amax) { o.dy_amax = gmax + 4 * n; o.x_amax = xmax + 4 * n; }
            o.v_have = pl.b[n].keep ? ws + l.o_vkeep[n] : nullptr;
            AFI_TRY(wino_wgrad(cx, gy, xin, N, H, W, co, ci, gr->w[n], 1.f, scratch + s.o_wino2, s.n_wino, sd, o));
        } else if (gr->w[n]) AFI_TRY(wgrad_launch(cx, conv_wgrad_desc(gy, xin, N, H, W, co, ci, gr->w[n], 1.f), sd));
        float* gx = n > 0 ? scratch + s.o_g[n - 1] : dx;   // d(activation of block n - 1), or dx
        if (gx && wino) {
            WinoConvOpt o;
            o.in_amax = bwd_amax ? gmax + 4 * n : nullptr; o.in_amax_known = true;
            AFI_TRY(wino_conv(cx, kWinoDgrad, gy, N, H, W, co, prm->w[n], ci, nullptr, dense_view(gx, H, W, ci), null_view(), scratch + s.o_wino, s.n_wino, part_,
                              part_n_, st, o));
        } else if (gx) {
            AFI_TRY(PG(conv_dgrad_desc(gy, N, H, W, co, prm->w[n], ci, dense_view(gx, H, W, ci)), 1));
        }
    }
    fk.join();
    return AFI_OK;
}

extern "C" {

int afi_discriminator_fwd(afi_ctx_t* ctx, const afi_disc_params_t* prm, afi_view_t xv, int N, int H, int W, float* logits, int training, float* ws,
                          long long ws_floats, void* stream) {
    return disc_fwd(ctx, prm, xv, N, H, W, 1, logits, training, ws, ws_floats, stream);
}
int afi_discriminator_bwd(afi_ctx_t* ctx, const afi_disc_params_t* prm, const afi_disc_params_t* gr, afi_view_t xv, int N, int H, int W, const float* ws,
                          const float* dlogits, float* dx, float* scratch, long long scratch_floats, void* stream) {
    return disc_bwd(ctx, prm, gr, xv, N, H, W, 1, ws, dlogits, dx, scratch, scratch_floats, stream);
}
int afi_discriminator_fwd_paired(afi_ctx_t* ctx, const afi_disc_params_t* prm, afi_view_t xv, int N, int H, int W, float* logits, int training, float* ws,
                                 long long ws_floats, void* stream) {
    return disc_fwd(ctx, prm, xv, N, H, W, 2, logits, training, ws, ws_floats, stream);
}
int afi_discriminator_bwd_paired(afi_ctx_t* ctx, const afi_disc_params_t* prm, const afi_disc_params_t* gr, afi_view_t xv, int N, int H, int W, const float* ws,
                                 const float* dlogits, float* dx, float* scratch, long long scratch_floats, void* stream) {
    return disc_bwd(ctx, prm, gr, xv, N, H, W, 2, ws, dlogits, dx, scratch, scratch_floats, stream);
}

}  // extern "C"
