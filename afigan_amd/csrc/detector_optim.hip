// The detector's optimiser step (afigan_amd/detector_optim.py): torch.optim.SGD as detectron2 v0.1.1's build_optimizer configures
// it, for every trainable tensor of the detector in ONE launch over a device table of afi_det_sgd_desc_t, with the FrozenBN refold of the
// trainable frozen.Conv2d weights in the same pass.
//   per element, fp32:  d = fmaf(wd, p, g * gscale);  m = fmaf(momentum, m, d);  p = fmaf(-lr, m, p)          (lr, wd per tensor)
//   fold entries:       fold_out = (float)((double)p_new * s64[o])  -- frozen.fold_conv's expression, one fp64 product rounded once,
//                       k = 1 into [O][I] (the parameter's own order), k = 3 from the parameter's [O][I][3][3] into the kernels' [O][3][3][I].
// Work is cut into units.  A plain or k = 1 tensor: DS_UNIT consecutive elements per unit, 16-byte loads and stores when p, g, m (and fold_out)
// are 16-byte aligned and four elements remain, scalar otherwise (tails, unaligned views).  A k = 3 fold tensor: DS_WAVES (o, 32 input
// channels) pieces per unit, one per wave: the wave updates the piece's 32 * 9 consecutive floats of p and m and parks w' in a private LDS
// tile, then writes the tile out as 9 rows of 32 floats -- afi_frozen_wgrad_unfold's shape run the other way, whole lines on both sides.
// Two grids walk the same units (afi_detector_sgd_step): (<= 512, ntensors) with a block striding over its tensor's units, or a flat grid
// striding over all units with the tensor found by bisection of the unit prefix.  Every element has one owner: no atomics, bit-identical
// between runs and between the two grids.
#include "../../include/afigan_hip.h"
#include "afi_common.h"

#define DS_THREADS 256
#define DS_ITERS 4
#define DS_UNIT (DS_THREADS * 4 * DS_ITERS)     // elements of a plain unit
#define DS_CH 32                                // input channels per k = 3 piece
#define DS_WAVES (DS_THREADS / 64)              // k = 3 pieces per unit

// the one statement of how a tensor is cut: the launcher's grids, the Python side's prefix and both kernels' loops read it
__host__ __device__ static inline long long ds_units(long long n, int O, int I, int k, int fold) {
    if (n <= 0) return 0;
    if (fold && k == 3) return ((long long)O * ((I + DS_CH - 1) / DS_CH) + DS_WAVES - 1) / DS_WAVES;
    return (n + DS_UNIT - 1) / DS_UNIT;
}

long long afi_detector_sgd_units(long long n, int O, int I, int k, int fold) { return ds_units(n, O, I, k, fold); }

__device__ __forceinline__ void ds_update(float& p, float g, float& m, float lr, float wd, float mom, float gscale) {
    const float d = fmaf(wd, p, g * gscale);
    m = fmaf(mom, m, d);
    p = fmaf(-lr, m, p);
}

__device__ __forceinline__ bool ds_al16(const void* q) { return ((unsigned long long)q & 15ull) == 0; }

// one unit of a plain / k = 1 tensor
__device__ __forceinline__ void ds_plain_unit(const afi_det_sgd_desc_t& d, long long u, float mom, float gscale) {
    const bool fold = d.fold_out != nullptr;
    const bool vec = ds_al16(d.p) && ds_al16(d.g) && ds_al16(d.m) && (!fold || (ds_al16(d.fold_out) && d.I >= 4));      // (uniform; I >= 4: four elements span two rows at most)
    const long long base = u * DS_UNIT;
#pragma unroll
    for (int it = 0; it < DS_ITERS; ++it) {
        const long long i = base + ((long long)it * DS_THREADS + threadIdx.x) * 4;
        if (i >= d.n) continue;
        if (vec && i + 4 <= d.n) {
            float4 p = *(const float4*)(d.p + i), m = *(const float4*)(d.m + i);
            const float4 g = *(const float4*)(d.g + i);
            ds_update(p.x, g.x, m.x, d.lr, d.wd, mom, gscale);
            ds_update(p.y, g.y, m.y, d.lr, d.wd, mom, gscale);
            ds_update(p.z, g.z, m.z, d.lr, d.wd, mom, gscale);
            ds_update(p.w, g.w, m.w, d.lr, d.wd, mom, gscale);
            *(float4*)(d.m + i) = m;
            *(float4*)(d.p + i) = p;
            if (fold) {
                const long long o = i / d.I, r = i - o * d.I;                       // elements i .. i + 3 sit in row o or o + 1
                const double s0 = d.s64[o], s1 = r + 3 >= d.I ? d.s64[min(o + 1, (long long)d.O - 1)] : s0;
                float4 f;
                f.x = (float)((double)p.x * s0);
                f.y = (float)((double)p.y * (r + 1 >= d.I ? s1 : s0));
                f.z = (float)((double)p.z * (r + 2 >= d.I ? s1 : s0));
                f.w = (float)((double)p.w * (r + 3 >= d.I ? s1 : s0));
                *(float4*)(d.fold_out + i) = f;
            }
        } else {
            const long long e = min(i + 4, d.n);
            for (long long j = i; j < e; ++j) {
                float p = d.p[j], m = d.m[j];
                ds_update(p, d.g[j], m, d.lr, d.wd, mom, gscale);
                d.m[j] = m;
                d.p[j] = p;
                if (fold) d.fold_out[j] = (float)((double)p * d.s64[j / d.I]);
            }
        }
    }
}

// one unit (DS_WAVES pieces) of a k = 3 fold tensor; called by every thread of the block (barriers inside)
__device__ __forceinline__ void ds_fold3_unit(const afi_det_sgd_desc_t& d, long long u, float mom, float gscale, float (*tile)[9][DS_CH + 1]) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int chunks = (d.I + DS_CH - 1) / DS_CH;
    const long long pieces = (long long)d.O * chunks, pc = u * DS_WAVES + wave;
    const bool live = pc < pieces;
    const int o = live ? (int)(pc / chunks) : 0;
    const int i0 = live ? (int)(pc - (long long)o * chunks) * DS_CH : 0;
    const int ni = live ? min(DS_CH, d.I - i0) : 0;
    const long long off = ((long long)o * d.I + i0) * 9;                            // the piece: 9 ni consecutive floats of p, g, m
    const int cnt = ni * 9;
    const bool vin = ds_al16(d.p) && ds_al16(d.g) && ds_al16(d.m) && (d.I & 3) == 0 && (cnt & 3) == 0;   // off % 4 == 0 then
    float (*tl)[DS_CH + 1] = tile[wave];
    if (vin) {
        for (int v = lane; v < cnt / 4; v += 64) {
            const long long i = off + 4 * v;
            float4 p = *(const float4*)(d.p + i), m = *(const float4*)(d.m + i);
            const float4 g = *(const float4*)(d.g + i);
            ds_update(p.x, g.x, m.x, d.lr, d.wd, mom, gscale);
            ds_update(p.y, g.y, m.y, d.lr, d.wd, mom, gscale);
            ds_update(p.z, g.z, m.z, d.lr, d.wd, mom, gscale);
            ds_update(p.w, g.w, m.w, d.lr, d.wd, mom, gscale);
            *(float4*)(d.m + i) = m;
            *(float4*)(d.p + i) = p;
            const float q[4] = {p.x, p.y, p.z, p.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int e = 4 * v + j, ii = e / 9, t = e - ii * 9;
                tl[t][ii] = q[j];
            }
        }
    } else {
        for (int e = lane; e < cnt; e += 64) {
            float p = d.p[off + e], m = d.m[off + e];
            ds_update(p, d.g[off + e], m, d.lr, d.wd, mom, gscale);
            d.m[off + e] = m;
            d.p[off + e] = p;
            const int ii = e / 9, t = e - ii * 9;
            tl[t][ii] = p;
        }
    }
    __syncthreads();
    if (live) {
        const double s = d.s64[o];
        float* dst = d.fold_out + (long long)o * 9 * d.I + i0;                      // row t of the piece at dst + t * I
        if (ni == DS_CH && (d.I & 3) == 0 && ds_al16(d.fold_out)) {
            for (int v = lane; v < 9 * (DS_CH / 4); v += 64) {
                const int t = v / (DS_CH / 4), ii = (v - t * (DS_CH / 4)) * 4;
                float4 f;
                f.x = (float)((double)tl[t][ii] * s);
                f.y = (float)((double)tl[t][ii + 1] * s);
                f.z = (float)((double)tl[t][ii + 2] * s);
                f.w = (float)((double)tl[t][ii + 3] * s);
                *(float4*)(dst + (long long)t * d.I + ii) = f;
            }
        } else {
            for (int e = lane; e < 9 * DS_CH; e += 64) {
                const int t = e / DS_CH, ii = e - t * DS_CH;
                if (ii < ni) dst[(long long)t * d.I + ii] = (float)((double)tl[t][ii] * s);
            }
        }
    }
    __syncthreads();
}

__device__ __forceinline__ bool ds_valid(const afi_det_sgd_desc_t& d) {
    if (d.n <= 0 || !d.p || !d.g || !d.m) return false;
    if (d.fold_out) return d.s64 && d.O > 0 && d.I > 0 && (d.k == 1 || d.k == 3) && d.n == (long long)d.O * d.I * d.k * d.k;
    return true;
}

// grid (<= 512, ntensors): a block strides over the units of tensor blockIdx.y
__global__ __launch_bounds__(DS_THREADS) void afi_detector_sgd_grid_kernel(const afi_det_sgd_desc_t* __restrict__ descs, float mom, float gscale) {
    __shared__ float tile[DS_WAVES][9][DS_CH + 1];
    const afi_det_sgd_desc_t d = descs[blockIdx.y];
    if (!ds_valid(d)) return;                                                       // (uniform)
    const bool f3 = d.fold_out && d.k == 3;
    const long long units = ds_units(d.n, d.O, d.I, d.k, d.fold_out != nullptr);
    for (long long u = blockIdx.x; u < units; u += gridDim.x) {                     // (uniform trip count)
        if (f3) ds_fold3_unit(d, u, mom, gscale, tile);
        else ds_plain_unit(d, u, mom, gscale);
    }
}

// flat grid: a block strides over all units; unit_off[t] = the first unit of tensor t, unit_off[ntensors] = their number
__global__ __launch_bounds__(DS_THREADS) void afi_detector_sgd_flat_kernel(const afi_det_sgd_desc_t* __restrict__ descs, const int* __restrict__ unit_off,
                                                                           int ntensors, float mom, float gscale) {
    __shared__ float tile[DS_WAVES][9][DS_CH + 1];
    const int total = unit_off[ntensors];
    for (int u = blockIdx.x; u < total; u += gridDim.x) {                           // (uniform)
        int lo = 0, hi = ntensors - 1;                                              // the last t with unit_off[t] <= u (an empty tensor is never it)
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (unit_off[mid] <= u) lo = mid; else hi = mid - 1;
        }
        const afi_det_sgd_desc_t d = descs[lo];
        if (!ds_valid(d)) continue;
        const long long lu = u - unit_off[lo];
        const bool f3 = d.fold_out && d.k == 3;
        const long long units = ds_units(d.n, d.O, d.I, d.k, d.fold_out != nullptr);
        if (lu >= units) continue;                                                  // (a prefix that claims more units than the tensor has)
        if (f3) ds_fold3_unit(d, lu, mom, gscale, tile);
        else ds_plain_unit(d, lu, mom, gscale);
    }
}

static int ds_check(const afi_det_sgd_desc_t* descs_host, int ntensors) {
    for (int t = 0; t < ntensors; ++t) {
        const afi_det_sgd_desc_t& d = descs_host[t];
        if (d.n < 0) return AFI_ERR_BAD_ARG;
        if (d.n == 0) continue;
        if (!d.p || !d.g || !d.m) return AFI_ERR_BAD_ARG;
        if (d.fold_out && (!d.s64 || (d.k != 1 && d.k != 3) || d.O <= 0 || d.I <= 0 || d.n != (long long)d.O * d.I * d.k * d.k)) return AFI_ERR_BAD_ARG;
    }
    return AFI_OK;
}

int afi_detector_sgd_step(const afi_det_sgd_desc_t* descs_host, const afi_det_sgd_desc_t* descs_dev, int ntensors, long long max_units,
                          const int* unit_off_dev, long long total_units, float momentum, float gscale, void* stream) {
    if (!descs_host || !descs_dev || ntensors <= 0 || ntensors > 65535) return AFI_ERR_BAD_ARG;
    if (ds_check(descs_host, ntensors) != AFI_OK) return AFI_ERR_BAD_ARG;
    if (unit_off_dev) {
        if (total_units < 0 || total_units > 0x7fffffffll) return AFI_ERR_BAD_ARG;
        if (total_units == 0) return AFI_OK;
        const unsigned gx = (unsigned)(total_units < 2048 ? total_units : 2048);
        hipLaunchKernelGGL(afi_detector_sgd_flat_kernel, dim3(gx), dim3(DS_THREADS), 0, (hipStream_t)stream, descs_dev, unit_off_dev, ntensors, momentum, gscale);
    } else {
        if (max_units < 0) return AFI_ERR_BAD_ARG;
        if (max_units == 0) return AFI_OK;
        const unsigned gx = (unsigned)(max_units < 512 ? max_units : 512);
        hipLaunchKernelGGL(afi_detector_sgd_grid_kernel, dim3(gx, (unsigned)ntensors), dim3(DS_THREADS), 0, (hipStream_t)stream, descs_dev, momentum, gscale);
    }
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}
