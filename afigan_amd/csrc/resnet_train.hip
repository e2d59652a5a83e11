// What training the ResNet bottom-up (afigan_amd/resnet_guide.py, _ResNetTrainFn) needs beyond the conv kernels it shares with the frozen
// forward and the heads' backward (afi_conv1x1_dgrad_act / afi_conv3x3_dgrad_act / afi_conv3x3_wino_dgrad_act and the weight-gradient GEMMs,
// csrc/nets.hip):
//   afi_frozen_wgrad_unfold     the convs run on weights folded with their FrozenBN, w' = w * s[o]; the weight-gradient GEMMs leave dw' in the
//                               kernels' [O][kh][kw][I] memory.  This is the chain rule back to the parameter and to its [O][I][kh][kw] memory,
//                               grad[o][i][t] = fmaf(s[o], dw'[o][t][i], grad[o][i][t]), for every trainable conv of the network in one launch.
// A wave owns one (o, 32 input channels) unit at a time: it reads the unit's k*k rows of 32 floats (128 B each) into a private LDS tile and
// writes the unit's 32 k*k consecutive floats of grad, so both sides move whole cache lines whatever k is.  Every element has one owner: no
// atomics, bit-identical between runs.
#include "../../include/afigan_hip.h"
#include "afi_common.h"

#define UF_CH 32                // input channels per unit
#define UF_WAVES 4              // units in flight per block

__global__ __launch_bounds__(64 * UF_WAVES) void afi_frozen_wgrad_unfold_kernel(const afi_unfold_desc_t* __restrict__ descs) {
    __shared__ float tile[UF_WAVES][9][UF_CH + 1];
    const afi_unfold_desc_t d = descs[blockIdx.y];
    const int k2 = d.k * d.k;
    if (d.O <= 0 || d.I <= 0 || (k2 != 1 && k2 != 9)) return;             // (uniform)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int chunks = (d.I + UF_CH - 1) / UF_CH;
    const long long units = (long long)d.O * chunks;
    for (long long base = (long long)blockIdx.x * UF_WAVES; base < units; base += (long long)gridDim.x * UF_WAVES) {   // (uniform trip count)
        const long long u = base + wave;
        const bool live = u < units;
        const int o = live ? (int)(u / chunks) : 0;
        const int i0 = live ? (int)(u - (long long)o * chunks) * UF_CH : 0;
        const int ni = live ? min(UF_CH, d.I - i0) : 0;
        const float* src = d.dw + ((long long)o * k2) * d.I + i0;         // row t of the unit at src + t * I
        for (int e = lane; e < k2 * UF_CH; e += 64) {
            const int t = e / UF_CH, ii = e - t * UF_CH;
            if (ii < ni) tile[wave][t][ii] = src[(long long)t * d.I + ii];
        }
        __syncthreads();
        if (live) {
            const float s = d.s[o];
            float* dst = d.grad + ((long long)o * d.I + i0) * k2;
            for (int e = lane; e < ni * k2; e += 64) {
                const int ii = e / k2, t = e - ii * k2;
                dst[e] = fmaf(s, tile[wave][t][ii], dst[e]);
            }
        }
        __syncthreads();
    }
}

int afi_frozen_wgrad_unfold(const afi_unfold_desc_t* descs_dev, int ntensors, long long max_oi, void* stream) {
    if (!descs_dev || ntensors <= 0 || ntensors > 65535 || max_oi <= 0) return AFI_ERR_BAD_ARG;
    long long gx = (max_oi + UF_WAVES - 1) / UF_WAVES;
    if (gx > 1024) gx = 1024;
    hipLaunchKernelGGL(afi_frozen_wgrad_unfold_kernel, dim3((unsigned)gx, (unsigned)ntensors), dim3(64 * UF_WAVES), 0, (hipStream_t)stream, descs_dev);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}
