// The inverse-CDF draw of the autoregressive samplers (PixelCNN, MADE): one wave holds the 256 logits of one unit, lane l the
// classes 4l .. 4l + 3.  Softmax in fp32 (max-shifted exponentials, inclusive scan of the lane sums), then k = min{k : cdf_k > u},
// clamped to 255; every lane returns the same k.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ int ar_inverse_cdf_pick(const float (&l)[4], float uu, int lane) {
    float m = fmaxf(fmaxf(l[0], l[1]), fmaxf(l[2], l[3]));
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    float e[4], run = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) { e[j] = expf(l[j] - m); run += e[j]; }
    float incl = run;                                   // inclusive scan of the lane sums
    for (int off = 1; off < 64; off <<= 1) {
        const float v = __shfl_up(incl, off);
        if (lane >= off) incl += v;
    }
    const float total = __shfl(incl, 63);
    const float inv = 1.f / total;
    float cum = incl - run;
    int pick = 256;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        cum += e[j];
        if (pick == 256 && cum * inv > uu) pick = lane * 4 + j;
    }
    for (int off = 32; off > 0; off >>= 1) pick = min(pick, __shfl_xor(pick, off));
    return pick > 255 ? 255 : pick;
}
