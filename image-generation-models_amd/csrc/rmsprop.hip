// The WGAN's optimizer tail (src/models/wgan.py): torch.optim.RMSprop over a flat fp32 buffer and the critic's weight clip.
// Both are HBM-bound, one launch each, float4 body + scalar tail, grid-stride under adam_kernel's block cap (elementwise.hip).
#include <math.h>
#include "common.h"

namespace {

constexpr int TPB = 256;
constexpr int BLOCK_CAP = 4096;                                  // adam_kernel's
inline int nblocks(size_t n) {
    size_t b = (n + TPB - 1) / TPB;
    return (int)(b < 1 ? 1 : (b > (size_t)BLOCK_CAP ? BLOCK_CAP : b));
}

// torch.optim.RMSprop defaults (no momentum, not centered, no weight decay): v = alpha v + (1 - alpha) g^2, p -= lr g / (sqrt(v) + eps).
// g = 0 with v = 0 gives 0 / eps = 0: the buffer's alignment padding and the pad lanes do not move.
__device__ __forceinline__ void rmsprop_one(float& p, float g, float& v, float lr, float alpha, float eps, float gs) {
    const float gr = g * gs;
    v = alpha * v + (1.f - alpha) * gr * gr;
    p -= lr * gr / (sqrtf(v) + eps);
}

__global__ void rmsprop_kernel(size_t n4, size_t n, float* __restrict__ p, const float* __restrict__ g, float* __restrict__ v, float lr,
                               float alpha, float eps, float gs) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        float4 pp = reinterpret_cast<float4*>(p)[i], gg = reinterpret_cast<const float4*>(g)[i], vv = reinterpret_cast<float4*>(v)[i];
        float* P = &pp.x; float* G = &gg.x; float* V = &vv.x;
#pragma unroll
        for (int j = 0; j < 4; ++j) rmsprop_one(P[j], G[j], V[j], lr, alpha, eps, gs);
        reinterpret_cast<float4*>(p)[i] = pp; reinterpret_cast<float4*>(v)[i] = vv;
    }
    // tail: at most 3 elements
    size_t i = n4 * 4 + blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i < n) {
        float pj = p[i], vj = v[i];
        rmsprop_one(pj, g[i], vj, lr, alpha, eps, gs);
        p[i] = pj; v[i] = vj;
    }
}

// torch.clamp_: comparisons, not fminf / fmaxf -- both comparisons are false for a NaN, which therefore stays; -0.0 is inside any
// range that holds 0 and stays -0.0.
__device__ __forceinline__ float clamp_one(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }

__global__ void clamp_kernel(size_t n4, size_t n, float* __restrict__ p, float lo, float hi) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        float4 pp = reinterpret_cast<float4*>(p)[i];
        pp.x = clamp_one(pp.x, lo, hi); pp.y = clamp_one(pp.y, lo, hi); pp.z = clamp_one(pp.z, lo, hi); pp.w = clamp_one(pp.w, lo, hi);
        reinterpret_cast<float4*>(p)[i] = pp;
    }
    // tail: at most 3 elements, or the whole range when it does not start on a 16-byte boundary (n4 = 0)
    for (size_t i = n4 * 4 + blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        p[i] = clamp_one(p[i], lo, hi);
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int mi_rmsprop_step(size_t n, float* p, const float* g, float* v, float lr, float alpha, float eps, float gscale, void* stream) {
    MI_REQUIRE(n > 0 && p && g && v, "bad argument");
    MI_REQUIRE((((uintptr_t)p | (uintptr_t)g | (uintptr_t)v) & 15) == 0, "buffers must be 16-byte aligned");
    const size_t n4 = n / 4;
    hipLaunchKernelGGL(rmsprop_kernel, dim3(nblocks(n4 ? n4 : 1)), dim3(TPB), 0, ST, n4, n, p, g, v, lr, alpha, eps, gscale);
    MI_LAUNCH_CHECK();
    return 0;
}

extern "C" int mi_clamp_inplace(size_t n, float* p, float lo, float hi, void* stream) {
    MI_REQUIRE(n > 0 && p, "bad argument");
    MI_REQUIRE(lo <= hi, "needs lo <= hi");
    MI_REQUIRE((((uintptr_t)p) & 3) == 0, "buffer must be 4-byte aligned");
    // a sub-range of a larger buffer may start off a 16-byte boundary: it goes through the scalar loop as a whole
    const bool al16 = (((uintptr_t)p) & 15) == 0;
    const size_t n4 = al16 ? n / 4 : 0;
    const size_t work = n4 > n - 4 * n4 ? n4 : n - 4 * n4;
    hipLaunchKernelGGL(clamp_kernel, dim3(nblocks(work ? work : 1)), dim3(TPB), 0, ST, n4, n, p, lo, hi);
    MI_LAUNCH_CHECK();
    return 0;
}
