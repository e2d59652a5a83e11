// Forward 1x1 convolution of FROZEN weights on the bf16 matrix cores (bf16x6: the arithmetic of afi_pix_gemm_wk6, csrc/smallmap.hip), for the
// large maps of the frozen guides:  out = act(alpha * conv1x1(x, w) + bias + add_scale * add),  fp32 in memory on both sides.
//   * The weights arrive as the wk6 fragment image (AFI_WK6_STAGE_BYTES per (32 columns, 32 channels): [n half][hi | mid | lo][lane] x 16 B),
//     built ONCE per weight by afi_conv1x1_frozen_image (the builder of smallmap.hip): a lane's operand of one (n half, part) is one 16-byte
//     buffer load straight into the register the MFMA reads.
//   * A block of four waves owns 64 pixel rows x BN = 64 NJ output columns (NJ = 1, 2, 4: the host plan takes the widest tile whose grid still
//     fills the chip).  The activations are read ONCE per block and K chunk (KC = 128, 64 or 32 channels, whichever divides Cin), coalesced --
//     adjacent lanes read adjacent 16 bytes of a pixel's channels --, split ONCE into hi / mid / lo and kept pre-split in LDS in fragment order
//     (3 x 64 x KC x 2 B <= 48 KB: two blocks per CU, so one block's load / split / store phases run under the other's MFMAs).  The next chunk's
//     loads are in flight under the current chunk's MFMAs.
//   * Every wave then sweeps its 16 NJ columns: per 32-channel K step twelve LDS fragment reads (4 row groups x 3 parts) feed 24 NJ MFMAs; the
//     weight fragments of the next (K step, n half) are requested behind the MFMAs of the current one.
//   * The MFMA computes the TRANSPOSED tile (weights as its row operand, pixels as its column operand: both fragments have the same register
//     layout, so this is only the argument order): a lane then holds four consecutive output channels of one pixel and the epilogue reads bias /
//     addend and stores with 16-byte accesses, without a trip through LDS.
//   * Products and their order per accumulator are those of afi_wk6_body: al*bh, ah*bl, am*bm, am*bh, ah*bm, ah*bh (smallest first), K steps in
//     ascending order.  No atomics, no split K, nothing allocated, no synchronisation: a launch is bit-reproducible and capturable.
// The N tiles of one row tile are adjacent logical blocks on one XCD, so the re-reads of its activations hit that XCD's L2.
#include "afi_common.h"
#include "afi_launch.h"
#include "afi_bf16_split.h"

#define AFI_F1_ROWS 64
struct AfiFrozen1x1 {
    const float* x; long long x_sN, x_sH, x_sW;             // the input view (elements); x_dense: row m of the GEMM starts at m * x_sW
    const unsigned char* image; const float* bias; const float* add; float* out;
    unsigned x_bytes, o_bytes, i_bytes;                     // buffer extents (the plan keeps each below 2 GB)
    int x_dense, M, HW, W, Cin, Cout, kc, ntile_n, nst;     // nst: 32-channel K stages of the image = Cin / 32
    float alpha, add_scale; int act;
};

__device__ __forceinline__ int afi_f1_logical_id() {        // XCD-contiguous logical block ids (bijective for any grid; as smallmap.hip's)
    const int nwg = gridDim.x, qq = nwg >> 3, rr = nwg & 7, xcd = blockIdx.x & 7;
    return (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + (int)(blockIdx.x >> 3);
}

// LDS: part pt at pt * (kc * 128) bytes; inside a part the fragment of (K step ks, row group mi) is 1 KB: lane (lq, l15) at 16 (16 lq + (l15 ^ 4 lq)).
// (The XOR spreads the four lq groups a staging wave writes at once over all banks; a fragment read stays one contiguous 256 B per 16 lanes.)
template <int NJ>
__global__ __launch_bounds__(256, 2) void afi_frozen1x1_kernel(const AfiFrozen1x1 p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, lq = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lb = afi_f1_logical_id();
    const int tile_m = lb / p.ntile_n, tile_n = lb - tile_m * p.ntile_n;
    const int m0 = tile_m * AFI_F1_ROWS;
    const int kc = p.kc, nks = kc >> 5, nchunks = p.Cin / kc, part_bytes = kc * 128;
    const int pl = kc == 128 ? 5 : (kc == 64 ? 4 : 3);       // log2 of the 16-byte pieces per row and chunk
    const int iters = 1 << (pl - 2);                         // 64 rows x 2^pl pieces over 256 threads
    const __amdgpu_buffer_rsrc_t rsrc_x = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, 0, p.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsrc_b = __builtin_amdgcn_make_buffer_rsrc((void*)p.image, 0, p.i_bytes, 0x00020000);

    // ---- staging: item (row, q) = 16 bytes q of row's chunk; thread tid takes items tid + 256 i
    const int q = tid & ((1 << pl) - 1), r0 = tid >> pl, rstep = 256 >> pl;
    unsigned row_off[8];                                     // byte offset of the row's first channel (0xFFFFFFFF: past M, reads zeros)
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int m = m0 + r0 + i * rstep;
        unsigned off = 0xFFFFFFFFu;
        if (i < iters && m < p.M) {
            if (p.x_dense) off = 4u * (unsigned)m * (unsigned)p.x_sW;
            else {
                const int img = m / p.HW, rem = m - img * p.HW, y = rem / p.W, xx = rem - y * p.W;
                off = 4u * (unsigned)(img * p.x_sN + y * p.x_sH + xx * p.x_sW);
            }
        }
        row_off[i] = off;
    }
    u32x4 a_raw[8];
    auto load_chunk = [&](int c) {
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (i < iters)
                a_raw[i] = __builtin_amdgcn_raw_buffer_load_b128(rsrc_x, row_off[i] == 0xFFFFFFFFu ? 0xFFFFFFFFu : row_off[i] + (unsigned)(4 * (c * kc) + 16 * q), 0, 0);
    };
    const int s_ks = q >> 3, s_lq = (q >> 1) & 3, s_half = q & 1;
    auto split_store = [&]() {
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (i < iters) {
                const int row = r0 + i * rstep, mi = row >> 4, rl = row & 15;
                const f32x4 v = __builtin_bit_cast(f32x4, a_raw[i]);
                unsigned h0, m0_, l0, h1, m1_, l1;
                afi_split3_pair(v[0], v[1], h0, m0_, l0);
                afi_split3_pair(v[2], v[3], h1, m1_, l1);
                unsigned char* d = lds + ((s_ks * 4 + mi) * 64 + 16 * s_lq + (rl ^ (4 * s_lq))) * 16 + 8 * s_half;
                *(u32x2*)d = u32x2{h0, h1};
                *(u32x2*)(d + part_bytes) = u32x2{m0_, m1_};
                *(u32x2*)(d + 2 * part_bytes) = u32x2{l0, l1};
            }
    };

    // ---- this wave's n halves: h = h0 + j, 16 columns each; beyond Cout (a ragged last N tile): loads clamp to half 0, nothing is stored
    const int h0 = (tile_n * 4 + wave) * NJ;
    const int frag_off = 16 * (16 * lq + (l15 ^ (4 * lq)));
    u32x4 bq[3];
    auto load_b = [&](int j, int stage) {                    // (j: compile-time at every call site)
        int h = h0 + j;
        if (h * 16 >= p.Cout) h = 0;
        const int st = stage < p.nst ? stage : p.nst - 1;    // (the request behind the last MFMAs re-reads the last stage and is never used)
        const int soff = ((h >> 1) * p.nst + st) * AFI_WK6_STAGE_BYTES + 3 * (h & 1) * 1024;
#pragma unroll
        for (int pt = 0; pt < 3; ++pt) bq[pt] = __builtin_amdgcn_raw_buffer_load_b128(rsrc_b, (unsigned)(16 * lane + pt * 1024), soff, 0);
    };
    f32x4 acc[NJ][4];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) acc[j][mi] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto mfma = [](u32x4 wf, u32x4 xf, f32x4 c) -> f32x4 {   // rows: output channels, columns: pixels
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wf), __builtin_bit_cast(bf16x8, xf), c, 0, 0, 0);
    };

    load_chunk(0);
    load_b(0, 0);
    for (int c = 0; c < nchunks; ++c) {
        split_store();
        __syncthreads();
        if (c + 1 < nchunks) load_chunk(c + 1);              // in flight under this chunk's MFMAs
        for (int ks = 0; ks < nks; ++ks) {
            u32x4 fa[4][3];                                  // [row group][hi | mid | lo]
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                for (int pt = 0; pt < 3; ++pt) fa[mi][pt] = *(const u32x4*)(lds + pt * part_bytes + (ks * 4 + mi) * 1024 + frag_off);
            const int stage = c * nks + ks;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const u32x4 bh = bq[0], bm = bq[1], bl = bq[2];
                if (j + 1 < NJ) load_b(j + 1, stage); else load_b(0, stage + 1);
                // per accumulator: smallest terms first; consecutive MFMAs go to different accumulators
#pragma unroll
                for (int mi = 0; mi < 4; ++mi) acc[j][mi] = mfma(bh, fa[mi][2], acc[j][mi]);
#pragma unroll
                for (int mi = 0; mi < 4; ++mi) acc[j][mi] = mfma(bl, fa[mi][0], acc[j][mi]);
#pragma unroll
                for (int mi = 0; mi < 4; ++mi) acc[j][mi] = mfma(bm, fa[mi][1], acc[j][mi]);
#pragma unroll
                for (int mi = 0; mi < 4; ++mi) acc[j][mi] = mfma(bh, fa[mi][1], acc[j][mi]);
#pragma unroll
                for (int mi = 0; mi < 4; ++mi) acc[j][mi] = mfma(bm, fa[mi][0], acc[j][mi]);
#pragma unroll
                for (int mi = 0; mi < 4; ++mi) acc[j][mi] = mfma(bh, fa[mi][0], acc[j][mi]);
            }
        }
        if (c + 1 < nchunks) __syncthreads();                // every wave has read this chunk's fragments before the next one overwrites them
    }

    // ---- epilogue: acc[j][mi][r] = channel 16 (h0 + j) + 4 lq + r of pixel m0 + 16 mi + l15
    const __amdgpu_buffer_rsrc_t rsrc_o = __builtin_amdgcn_make_buffer_rsrc((void*)p.out, 0, p.o_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsrc_r = __builtin_amdgcn_make_buffer_rsrc((void*)p.add, 0, p.add ? p.o_bytes : 0u, 0x00020000);
    const float slope = p.act == 1 ? AFI_LRELU_SLOPE : 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int col = 16 * (h0 + j) + 4 * lq;
        if (16 * (h0 + j) >= p.Cout) break;                  // (wave-uniform)
        f32x4 bias = {0.f, 0.f, 0.f, 0.f};
        if (p.bias) bias = *(const f32x4*)(p.bias + col);
        unsigned off[4];
        f32x4 r[4];
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
            const int m = m0 + 16 * mi + l15;
            off[mi] = m < p.M ? 4u * ((unsigned)m * (unsigned)p.Cout + (unsigned)col) : 0xFFFFFFFFu;
            r[mi] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (p.add) r[mi] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_r, off[mi], 0, 0));
        }
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
            f32x4 v = p.alpha * acc[j][mi];
            v += bias;
            if (p.add) v += p.add_scale * r[mi];
            if (p.act) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : v[e] * slope;
            }
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rsrc_o, off[mi], 0, 0);
        }
    }
}

// ------------------------------------------------------------------------------------------------ host side
// Eligibility, tile form and grid from the shape and the strides alone (no device): AFI_OK and plan[] filled, AFI_ERR_UNSUPPORTED for what the
// kernel does not take (the caller runs afi_conv1x1_fwd), AFI_ERR_BAD_ARG for a shape that is none.
//   x:   every s-th pixel (s >= 1, both directions) of a pixel-major tensor of Cin channels: x_sW = s Cin, x_sH >= s ((W - 1) s + 1) Cin,
//        x_sN >= (H - 1) x_sH + ((W - 1) s + 1) Cin  (a channel slice of a wider tensor is NOT such a view and is refused);
//   out: dense pixel-major [N][H][W][Cout], add (if any) dense like out;
//   Cin % 32 == 0, Cout % 32 == 0; the byte extents of x, out and the image below 2 GB (the kernel's 32-bit buffer offsets).
extern "C" int afi_frozen1x1_plan(int N, int H, int W, int Cin, int Cout, long long x_sN, long long x_sH, long long x_sW, long long o_sN, long long o_sH,
                                  long long o_sW, int has_add, long long a_sN, long long a_sH, long long a_sW, long long* plan) {
    if (!plan || N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return AFI_ERR_BAD_ARG;
    for (int i = 0; i < AFI_FROZEN1X1_PLAN_SLOTS; ++i) plan[i] = 0;
    if ((Cin & 31) || (Cout & 31)) return AFI_ERR_UNSUPPORTED;
    const long long kLimit = 0x7FFFFFF0LL;
    const long long M = (long long)N * H * W;
    if (M > (1LL << 30)) return AFI_ERR_UNSUPPORTED;
    if (x_sW < Cin || x_sW % Cin != 0) return AFI_ERR_UNSUPPORTED;
    const long long s = x_sW / Cin, row_span = ((long long)(W - 1) * s + 1) * Cin;
    if (H > 1 && x_sH < s * row_span) return AFI_ERR_UNSUPPORTED;
    if (N > 1 && x_sN < (long long)(H - 1) * x_sH + row_span) return AFI_ERR_UNSUPPORTED;
    if ((x_sN | x_sH | x_sW) & 3) return AFI_ERR_UNSUPPORTED;                                  // 16-byte loads
    if (x_sN < 0 || x_sH < 0) return AFI_ERR_UNSUPPORTED;
    const long long x_elems = (long long)(N - 1) * x_sN + (long long)(H - 1) * x_sH + (long long)(W - 1) * x_sW + Cin;
    if (x_elems * 4 >= kLimit) return AFI_ERR_UNSUPPORTED;
    if (o_sW != Cout || o_sH != (long long)W * Cout || o_sN != (long long)H * W * Cout) return AFI_ERR_UNSUPPORTED;
    if (has_add && (a_sW != o_sW || a_sH != o_sH || a_sN != o_sN)) return AFI_ERR_UNSUPPORTED;
    const long long o_bytes = M * Cout * 4;
    if (o_bytes >= kLimit) return AFI_ERR_UNSUPPORTED;
    const long long i_bytes = afi_wk6_image_bytes(Cout, Cin, 1, 1);
    if (i_bytes >= kLimit) return AFI_ERR_UNSUPPORTED;
    const bool dense = x_sH == (long long)W * x_sW && x_sN == (long long)H * x_sH;
    const long long ntm = (M + AFI_F1_ROWS - 1) / AFI_F1_ROWS;
    // the widest column tile (fewest re-reads and re-splits of the activations) whose grid still gives every CU two blocks
    int bn = 64;
    for (int cand = 256; cand > 64; cand >>= 1) {
        if (cand > ((Cout + 63) & ~63)) continue;
        if (ntm * ((Cout + cand - 1) / cand) >= 512) { bn = cand; break; }
    }
    const long long ntn = (Cout + bn - 1) / bn;
    if (ntm * ntn > 0x3FFFFFFFLL) return AFI_ERR_UNSUPPORTED;
    const int kc = (Cin % 128 == 0) ? 128 : ((Cin % 64 == 0) ? 64 : 32);
    plan[AFI_F1_M] = M; plan[AFI_F1_BM] = AFI_F1_ROWS; plan[AFI_F1_BN] = bn; plan[AFI_F1_KC] = kc;
    plan[AFI_F1_NTM] = ntm; plan[AFI_F1_NTN] = ntn; plan[AFI_F1_GRID] = ntm * ntn; plan[AFI_F1_LDS] = 3LL * AFI_F1_ROWS * kc * 2;
    plan[AFI_F1_XBYTES] = x_elems * 4; plan[AFI_F1_OBYTES] = o_bytes; plan[AFI_F1_IBYTES] = i_bytes; plan[AFI_F1_XDENSE] = dense ? 1 : 0;
    return AFI_OK;
}

extern "C" long long afi_frozen1x1_image_bytes(int Cout, int Cin) {
    if (Cout <= 0 || Cin <= 0 || (Cout & 31) || (Cin & 31)) return 0;
    return afi_wk6_image_bytes(Cout, Cin, 1, 1);
}

// one launch of the small-map image builder: the three bf16 planes of w [Cout][Cin] in the order the kernel's weight fragments are read
extern "C" int afi_conv1x1_frozen_image(afi_ctx_t* ctx, const float* w, int Cout, int Cin, void* image, long long image_bytes, void* stream) {
    (void)ctx;
    if (!w || !image || Cout <= 0 || Cin <= 0) return AFI_ERR_BAD_ARG;
    if ((Cout & 31) || (Cin & 31)) return AFI_ERR_UNSUPPORTED;
    if (image_bytes < afi_wk6_image_bytes(Cout, Cin, 1, 1)) return AFI_ERR_WORKSPACE;
    const AfiWk6ImgJob job = {w, (long long)Cin, 0, Cout, Cin, 1, 1, 0, (unsigned char*)image};
    return afi_launch_wk6_images(&job, 1, (hipStream_t)stream);
}

extern "C" int afi_conv1x1_frozen_fwd(afi_ctx_t* ctx, afi_view_t x, int N, int H, int W, int Cin, const void* image, const float* bias, int Cout, afi_view_t out,
                                      float alpha, afi_view_t add, float add_scale, int act, void* stream) {
    (void)ctx;
    if (!x.p || !out.p || !image || act < 0 || act > 2) return AFI_ERR_BAD_ARG;
    long long plan[AFI_FROZEN1X1_PLAN_SLOTS];
    AFI_TRY(afi_frozen1x1_plan(N, H, W, Cin, Cout, x.sN, x.sH, x.sW, out.sN, out.sH, out.sW, add.p != nullptr, add.sN, add.sH, add.sW, plan));
    if ((((uintptr_t)x.p | (uintptr_t)out.p | (uintptr_t)image | (uintptr_t)add.p | (uintptr_t)bias) & 15)) return AFI_ERR_UNSUPPORTED;
    AfiFrozen1x1 p;
    p.x = x.p; p.x_sN = x.sN; p.x_sH = x.sH; p.x_sW = x.sW;
    p.image = (const unsigned char*)image; p.bias = bias; p.add = add.p; p.out = out.p;
    p.x_bytes = (unsigned)plan[AFI_F1_XBYTES]; p.o_bytes = (unsigned)plan[AFI_F1_OBYTES]; p.i_bytes = (unsigned)plan[AFI_F1_IBYTES];
    p.x_dense = (int)plan[AFI_F1_XDENSE]; p.M = (int)plan[AFI_F1_M]; p.HW = H * W; p.W = W; p.Cin = Cin; p.Cout = Cout;
    p.kc = (int)plan[AFI_F1_KC]; p.ntile_n = (int)plan[AFI_F1_NTN]; p.nst = Cin / 32;
    p.alpha = alpha; p.add_scale = add_scale; p.act = act;
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)plan[AFI_F1_GRID]), block(256);
    const unsigned lds = (unsigned)plan[AFI_F1_LDS];
    void* prof = afi_prof_open(st, 23, 2.0 * (double)p.M * Cin * Cout, p.M, Cout, Cin);
    switch ((int)plan[AFI_F1_BN]) {
        case 256: hipLaunchKernelGGL(afi_frozen1x1_kernel<4>, grid, block, lds, st, p); break;
        case 128: hipLaunchKernelGGL(afi_frozen1x1_kernel<2>, grid, block, lds, st, p); break;
        default:  hipLaunchKernelGGL(afi_frozen1x1_kernel<1>, grid, block, lds, st, p); break;
    }
    afi_prof_close(prof);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}
