// Row-local latent discriminator of the adversarial autoencoder (reference src/models/aae.py:42-44: MLPEncoder(L, [256, 256], 1,
// norm_type="layer") of src/networks/basic.py:64-112):
//   x [N, L] -> Linear(L, 256) -> GroupNorm(1, 256) -> LeakyReLU(0.2) -> Linear(256, 256) -> GroupNorm(1, 256) -> LeakyReLU(0.2)
//            -> Linear(256, 1) = logit [N],  loss per row: binary cross-entropy on the logit ("vanilla") or (logit - t)^2 ("lsgan").
// Unlike csrc/latent_disc.hip there is no BatchNorm, so nothing depends on the batch: a row's logit is a function of that row alone and
// the whole network is ONE row-tiled launch in each direction.  What is left over are sums over the rows, which get a launch of their own:
//   forward   rows   : x -> fc1 -> LayerNorm -> LeakyReLU -> fc2 -> LayerNorm -> LeakyReLU -> fc3 -> logit, loss per row   (N / RT workgroups)
//             reduce : per-segment mean loss and mean logit, 0.5 (loss0 + loss1)                                            (1 workgroup, 5 numbers)
//   backward  rows   : d logit -> head -> LayerNorm backward -> fc2^T -> LayerNorm backward -> fc1^T = d x                  (N / RT workgroups)
//             params : every parameter gradient, one output element per thread                                             (32 + L/8 + 2)
// The batch is two segments: rows [0, N0) come from x0 with target0, rows [N0, N0 + N1) from x1 with target1 (N1 = 0 is allowed), so the
// real and the fake half of a discriminator step are one pass.  Row n of the pass is computed by the same instruction sequence
// whichever tile and segment it falls into: the logits of a joint pass equal those of two separate passes bit for bit.
// The conventions (weights input-major, fp32 tensors, fp64 sums in a fixed order) and the row-tile steps up to fc2 and back down from it
// (staging, fc1, LayerNorm-1 both ways, both fc2 contractions, fc1^T, and the fc2 / fc1 / vector branches of the parameter kernel) are
// csrc/latent_mlp.h, shared with csrc/latent_disc.hip.  Here are the segments, the second LayerNorm, the head and the losses, the tape
// and the entry points.  Both LayerNorms keep their statistics in fp64 (T = double in latent_mlp.h, which says why).
#include "latent_mlp.h"

namespace {

constexpr int NMAX = MI_LATENT_DISC_LN_NMAX;

// rows [0, N0) from x0 (pitch ld0), rows [N0, N0 + N1) from x1 (pitch ld1)
struct Seg { const float* x0; int ld0; const float* x1; int ld1; int N0, N1; float t0, t1; };
// tape (floats), N = N0 + N1: xhat1 [N][H] | h1 [N][H] | xhat2 [N][H] | rstd1 [N] | rstd2 [N] | logit [N] | loss [N]
struct Tape { float *xhat1, *h1, *xhat2, *rstd1, *rstd2, *logit, *loss; };
// workspace of the backward (floats): da2 [N][H] | dn1 [N][H] | da1 [N][H] | dl [N]
struct Ws { float *da2, *dn1, *da1, *dl; };

__device__ __forceinline__ const float* row_of(const Seg& s, int n) {
    return n < s.N0 ? s.x0 + (size_t)n * s.ld0 : s.x1 + (size_t)(n - s.N0) * s.ld1;
}

// loss of one row and its derivative by the logit.  mode 0: max(x, 0) - x t + log1p(exp(-|x|)) (finite for any finite x), d = sigmoid(x) - t;
// mode 1: (x - t)^2, d = 2 (x - t).
__device__ __forceinline__ double row_loss(int mode, double x, double t) {
    if (mode == 0) return fmax(x, 0.0) - x * t + log1p(exp(-fabs(x)));
    return (x - t) * (x - t);
}
__device__ __forceinline__ double row_dloss(int mode, double x, double t) {
    if (mode == 0) {
        const double e = exp(-fabs(x));                                      // in (0, 1]: no overflow at either end
        return (x >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e)) - t;
    }
    return 2.0 * (x - t);
}

// ------------------------------------------------------------------------------------------------------------------ forward
__global__ __launch_bounds__(TPB) void ldl_fwd_rows(int L, int mode, Seg s, Par p, Tape t) {
    __shared__ float xs[RT][LMAX];
    __shared__ __align__(16) float hs[RT][LDP];
    __shared__ double st[RT][2];
    const int N = s.N0 + s.N1;
    const int c = threadIdx.x, r0 = blockIdx.x * RT, lane = c & 63, wv = c >> 6;
    stage_rows(xs, r0, N, L, [=](int n, int j) { return row_of(s, n)[j]; });
    __syncthreads();
    float acc[RT];
    fc_in(xs, p.w1, p.b1, L, c, acc, hs);
    __syncthreads();
    ln_stats<double>(hs, st, lane, wv);
    __syncthreads();
    ln_act_store<double>(acc, st, p.g1[c], p.be1[c], r0, N, c, t.xhat1, t.h1, hs);
    if (c < RT && r0 + c < N) t.rstd1[r0 + c] = (float)st[c][1];
    __syncthreads();
    {
        double a2[RT];
        fc256(hs, p.w2, (double)p.b2[c], c, a2);
        __syncthreads();                                                     // every thread is done reading h1 from hs
#pragma unroll
        for (int r = 0; r < RT; ++r) { acc[r] = (float)a2[r]; hs[r][c] = acc[r]; }
    }
    __syncthreads();
    ln_stats<double>(hs, st, lane, wv);
    __syncthreads();
    {
        const float g = p.g2[c], be = p.be2[c];
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            const float xh = ln_xhat<double>(acc[r], st[r]);
            if (r0 + r < N) t.xhat2[(size_t)(r0 + r) * H + c] = xh;
            hs[r][c] = leaky(fmaf(g, xh, be));
        }
    }
    if (c < RT && r0 + c < N) t.rstd2[r0 + c] = (float)st[c][1];
    __syncthreads();
    for (int r = wv; r < RT; r += 4) {                                       // the head: one wave per row
        const float4 h = *reinterpret_cast<const float4*>(&hs[r][4 * lane]);
        const float4 w = *reinterpret_cast<const float4*>(&p.w3[4 * lane]);
        const double d = wave_sum_d(fma((double)h.w, (double)w.w, fma((double)h.z, (double)w.z, fma((double)h.y, (double)w.y, (double)h.x * w.x))));
        const int n = r0 + r;
        if (lane == 0 && n < N) {
            const float lg = (float)(d + (double)p.b3[0]);
            t.logit[n] = lg;
            t.loss[n] = (float)row_loss(mode, (double)lg, (double)(n < s.N0 ? s.t0 : s.t1));
        }
    }
}

// One workgroup: out5 = loss0, loss1, mean logit of segment 0, of segment 1, 0.5 (loss0 + loss1).  An empty second segment gives 0, 0.
// Thread c sums rows c, c + 256, ... of a segment upward, then the block sum: a fixed order.
__global__ __launch_bounds__(TPB) void ldl_fwd_reduce(int N0, int N1, Tape t, float* __restrict__ out5) {
    __shared__ double red[4];
    const int c = threadIdx.x;
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (int n = c; n < N0; n += TPB) { v[0] += t.loss[n]; v[2] += t.logit[n]; }
    for (int n = N0 + c; n < N0 + N1; n += TPB) { v[1] += t.loss[n]; v[3] += t.logit[n]; }
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = block_sum_256d(v[i], red);
    if (c == 0) {
        const double i0 = 1.0 / N0, i1 = N1 > 0 ? 1.0 / N1 : 0.0;
        const float l0 = (float)(v[0] * i0), l1 = (float)(v[1] * i1);
        out5[0] = l0;
        out5[1] = l1;
        out5[2] = (float)(v[2] * i0);
        out5[3] = (float)(v[3] * i1);
        out5[4] = (float)(0.5 * (v[0] * i0 + v[1] * i1));
    }
}

// ------------------------------------------------------------------------------------------------------------------ backward
// d (c0 loss0 + c1 loss1) / d logit[n] = c_seg / N_seg * row_dloss(logit[n], t_seg).  want_ws: keep what the parameter kernel reads; without it
// the workspace pointers in w are null.
__global__ __launch_bounds__(TPB) void ldl_bwd_rows(int L, int mode, Seg s, float c0, float c1, Par p, Tape t, Ws w, int want_ws,
                                                    float* __restrict__ dx0, int lddx, float xsc, int xacc) {
    __shared__ __align__(16) float ds[RT][LDP];
    __shared__ __align__(16) float xs[RT][LDP];
    __shared__ double st[RT][2];
    __shared__ float dls[RT];
    const int N = s.N0 + s.N1;
    const int c = threadIdx.x, r0 = blockIdx.x * RT, lane = c & 63, wv = c >> 6;
    if (c < RT) {
        const int n = r0 + c;
        float v = 0.f;
        if (n < N) {
            const bool first = n < s.N0;
            const double k = first ? (double)c0 / s.N0 : (double)c1 / s.N1;
            v = (float)(k * row_dloss(mode, (double)t.logit[n], (double)(first ? s.t0 : s.t1)));
            if (want_ws) w.dl[n] = v;
        }
        dls[c] = v;
    }
    __syncthreads();
    float dv[RT], xr[RT];
    {
        const float g2 = p.g2[c], be2 = p.be2[c], w3 = p.w3[c];
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            const int n = r0 + r;
            float xh = 0.f, d = 0.f;
            if (n < N) {
                xh = t.xhat2[(size_t)n * H + c];
                d = dls[r] * w3 * leaky_d(fmaf(g2, xh, be2)) * g2;            // d xhat2
            }
            dv[r] = d; xr[r] = xh;
        }
    }
    ln_backward<double>(dv, xr, t.rstd2, 1, r0, N, c, lane, wv, ds, xs, st, w.da2, dv);                   // d a2
#pragma unroll
    for (int r = 0; r < RT; ++r) ds[r][c] = dv[r];                           // the statistics pass finished reading ds before its last barrier
    __syncthreads();
    double a0[RT];
    fc256_t(ds, p.w2, c, a0);
    ln1_backward<double>(a0, p.g1[c], t.xhat1, t.h1, t.rstd1, 1, r0, N, c, lane, wv, ds, xs, st, w.dn1, w.da1, dv);
    if (!dx0 || r0 >= s.N0) return;                                          // uniform over the workgroup
    input_grad(dv, ds, p.w1, L, r0, s.N0, c, dx0, lddx, xsc, xacc);          // the input gradient goes to the first segment alone
}

// The workgroups of params_common, then one for d gamma2, d beta2, d W3, d b3.
__global__ __launch_bounds__(TPB) void ldl_bwd_params(int L, Seg s, Par p, Tape t, Ws w, Grad g, float ps, int pacc) {
    const int N = s.N0 + s.N1, c = threadIdx.x;
    if (params_common(blockIdx.x, N, L, [=](int n, int j) { return row_of(s, n)[j]; }, t.h1, t.xhat1, w.da2, w.dn1, w.da1, g, ps, pacc)) return;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    const float g2 = p.g2[c], be2 = p.be2[c], w3 = p.w3[c];
    for (int n = 0; n < N; ++n) {
        const float xh = t.xhat2[(size_t)n * H + c], pre = fmaf(g2, xh, be2), dl = w.dl[n];
        const double dn = (double)(dl * w3 * leaky_d(pre));                  // d of the second norm's output, as the row kernel forms it
        acc[0] = fma(dn, (double)xh, acc[0]);
        acc[1] += dn;
        acc[2] = fma((double)dl, (double)leaky(pre), acc[2]);
        acc[3] += dl;
    }
    put(g.g2 + c, acc[0], ps, pacc);
    put(g.be2 + c, acc[1], ps, pacc);
    put(g.w3 + c, acc[2], ps, pacc);
    if (c == 0) put(g.b3, acc[3], ps, pacc);
}

inline Tape tape_of(float* base, int N) {
    Tape t;
    const size_t nh = (size_t)N * H;
    t.xhat1 = base; t.h1 = base + nh; t.xhat2 = base + 2 * nh;
    t.rstd1 = base + 3 * nh; t.rstd2 = t.rstd1 + N; t.logit = t.rstd2 + N; t.loss = t.logit + N;
    return t;
}

const char* const SHAPE_MSG = "shape not supported (H == 256, 1 <= L <= 64, N0 >= 1, N1 >= 0, N0 + N1 <= MI_LATENT_DISC_LN_NMAX)";

int seg_of(int N0, int N1, int L, const float* x0, int ld0, const float* x1, int ld1, float t0, float t1, Seg* s) {
    if (!x0 || ld0 < L) return -1;
    if (N1 > 0 && (!x1 || ld1 < L)) return -1;
    *s = Seg{x0, ld0, N1 > 0 ? x1 : nullptr, N1 > 0 ? ld1 : 0, N0, N1, t0, t1};
    return 0;
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int mi_latent_disc_ln_supported(int N0, int N1, int L, int Hd) {
    if (Hd != H) return mi_set_error(0, "mi_latent_disc_ln: hidden width %d (only 256 is built)", Hd), 0;
    if (L < 1 || L > LMAX) return mi_set_error(0, "mi_latent_disc_ln: latent width %d outside [1, 64]", L), 0;
    if (N0 < 1 || N1 < 0) return mi_set_error(0, "mi_latent_disc_ln: segments of %d and %d rows (the first needs 1, the second 0)", N0, N1), 0;
    if ((long long)N0 + N1 > NMAX)
        return mi_set_error(0, "mi_latent_disc_ln: %lld rows, more than %d (the parameter sums walk the rows serially)", (long long)N0 + N1, NMAX), 0;
    return 1;
}

extern "C" size_t mi_latent_disc_ln_tape_floats(int N) { return N > 0 ? 3 * (size_t)N * H + 4 * (size_t)N : 0; }
extern "C" size_t mi_latent_disc_ln_workspace_floats(int N) { return N > 0 ? 3 * (size_t)N * H + (size_t)N : 0; }

extern "C" int mi_latent_disc_ln_fwd(int N0, int N1, int L, int Hd, const float* x0, int ld0, const float* x1, int ld1,
                                     const float* const* params, int loss_mode, float target0, float target1, float* tape, float* out5,
                                     void* stream) {
    MI_REQUIRE(mi_latent_disc_ln_supported(N0, N1, L, Hd) == 1, SHAPE_MSG);
    MI_REQUIRE(params && tape && out5, "bad argument");
    MI_REQUIRE(loss_mode == 0 || loss_mode == 1, "loss_mode: 0 (vanilla) or 1 (lsgan)");
    Seg s;
    MI_REQUIRE(seg_of(N0, N1, L, x0, ld0, x1, ld1, target0, target1, &s) == 0, "input: x0 (ld0 >= L), and x1 (ld1 >= L) when N1 > 0");
    MI_REQUIRE(all_ten_set(params), "a parameter pointer is null");
    MI_REQUIRE(aligned16(tape) && aligned16(params[8]), "tape, fc3 weight: 16-byte alignment");
    const Par p = par_of(params);
    const int N = N0 + N1;
    Tape t = tape_of(tape, N);
    hipLaunchKernelGGL(ldl_fwd_rows, dim3((N + RT - 1) / RT), dim3(TPB), 0, ST, L, loss_mode, s, p, t);
    MI_LAUNCH_CHECK();
    hipLaunchKernelGGL(ldl_fwd_reduce, dim3(1), dim3(TPB), 0, ST, N0, N1, t, out5);
    MI_LAUNCH_CHECK();
    return 0;
}

extern "C" int mi_latent_disc_ln_bwd(int N0, int N1, int L, int Hd, const float* x0, int ld0, const float* x1, int ld1,
                                     const float* const* params, int loss_mode, float target0, float target1, float c0, float c1,
                                     const float* tape, float* workspace, float* const* grads, float param_scale, int accumulate_params,
                                     float* dx0, int lddx, float dx_scale, int accumulate_dx, void* stream) {
    MI_REQUIRE(mi_latent_disc_ln_supported(N0, N1, L, Hd) == 1, SHAPE_MSG);
    MI_REQUIRE(params && tape, "bad argument");
    MI_REQUIRE(loss_mode == 0 || loss_mode == 1, "loss_mode: 0 (vanilla) or 1 (lsgan)");
    MI_REQUIRE(grads || dx0, "neither parameter gradients nor an input gradient asked for");
    MI_REQUIRE(!grads || workspace, "parameter gradients need the workspace");
    MI_REQUIRE(!dx0 || lddx >= L, "dx0: lddx >= L");
    Seg s;
    MI_REQUIRE(seg_of(N0, N1, L, x0, ld0, x1, ld1, target0, target1, &s) == 0, "input: x0 (ld0 >= L), and x1 (ld1 >= L) when N1 > 0");
    MI_REQUIRE(all_ten_set(params) && (!grads || all_ten_set(grads)), "a parameter / gradient pointer is null");
    MI_REQUIRE(aligned16(tape) && (!workspace || aligned16(workspace)) && aligned16(params[0]) && aligned16(params[4]),
               "tape, workspace, fc1 / fc2 weights: 16-byte alignment");
    const Par p = par_of(params);
    const Grad g = grad_of(grads);
    const int N = N0 + N1;
    Tape t = tape_of(const_cast<float*>(tape), N);
    Ws w = {};
    if (grads) {
        const size_t nh = (size_t)N * H;
        w.da2 = workspace; w.dn1 = workspace + nh; w.da1 = workspace + 2 * nh; w.dl = workspace + 3 * nh;
    }
    hipLaunchKernelGGL(ldl_bwd_rows, dim3((N + RT - 1) / RT), dim3(TPB), 0, ST, L, loss_mode, s, c0, c1, p, t, w, grads ? 1 : 0, dx0, lddx,
                       dx_scale, accumulate_dx ? 1 : 0);
    MI_LAUNCH_CHECK();
    if (grads) {
        hipLaunchKernelGGL(ldl_bwd_params, dim3(NB_W2 + (L + KT - 1) / KT + 2), dim3(TPB), 0, ST, L, s, p, t, w, g, param_scale,
                           accumulate_params ? 1 : 0);
        MI_LAUNCH_CHECK();
    }
    return 0;
}
