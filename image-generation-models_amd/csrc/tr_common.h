// Shared pieces of the LDS-DMA / transposing-read weight-gradient kernels: wgrad_tr.hip (3x3), wgrad1x1_tr.hip (1x1 and the
// exact-fp32 stride-2 taps) and wgrad_s2_tr.hip (stride 2).  The three kinds differ in their contraction loops; what surrounds them is
// here, once: the host planner (balance_shares, kslices, batch_layout, ws_ok), the workgroup -> problem scans, the XCD rank map and the
// fixed-order k-slice sum of the reduce kernels.  (conv_pw.hip uses the LDS-DMA and transposing-read primitives at the bottom.)
#pragma once
#include <stdlib.h>
#include "common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

template <int I, int N, class F> __device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) { f(std::integral_constant<int, I>{}); static_for<I + 1, N>(f); }
}

// One launch = up to MAXP independent weight-gradient problems, each on its own share of the workgroups.  A 3x3 layer's partial-tile
// volume is (its workgroups) x 288 KB: eight layers side by side on 32 CUs each write an eighth of what one layer on 256 CUs
// writes (75 MB) for the same MFMA work, and layers with >= 32 tiles need no k-slices at all (they add into dW directly).
// Each kind has its own argument struct (TrArgs, W1Args, S2Args) and batch { Args p[MAXP]; int n; }; what the code below needs of them:
//   int total, sps, splits;   steps of 64 pixels over the whole batch, steps per k-slice, k-slices
//   int wg0, tile0;           first workgroup of the problem in the launch, first tile in the reduce launch
//   float* ws;                the problem's partial tiles [k-slice][tile][tile_floats()] (splits > 1)
//   int xcd_map;              workgroup -> (k-slice, tile) such that the tiles of a k-slice share an XCD (the rule is the kind's)
//   tiles(), tile_floats()    tiles of one k-slice, floats of one partial tile
constexpr int MAXP = 8;

// Workgroups per problem of a batched launch: every problem gets whole k-slices (a multiple of its tile count), at most `target`
// workgroups in total (one round of the chip), and the launch lasts as long as its slowest workgroup -- so slices are handed out
// greedily to the problem whose workgroups currently carry the most work each.  (Shares proportional to the work, rounded down to
// whole slices, left a 24-tile layer with 48 of the 70 workgroups it was due: the whole launch ran 1.46x longer.)
inline void balance_shares(int n, const double* work, const long* tiles, long target, long* wgs) {
    long total = 0;
    for (int i = 0; i < n; ++i) { wgs[i] = tiles[i]; total += tiles[i]; }
    for (;;) {
        int best = -1; double worst = 0;
        for (int i = 0; i < n; ++i) {
            const double per = work[i] / (double)wgs[i];
            if (per > worst && total + tiles[i] <= target) { worst = per; best = i; }
        }
        if (best < 0) break;
        // stop when the most loaded problem cannot be relieved: further slices for the others would not shorten the launch
        double top = 0;
        for (int i = 0; i < n; ++i) top = work[i] / (double)wgs[i] > top ? work[i] / (double)wgs[i] : top;
        if (worst < top) break;
        wgs[best] += tiles[best]; total += tiles[best];
    }
}

// k-slices of one problem (a.total steps, a.tiles() tiles) that is given `wgs` workgroups: a.sps, a.splits
template <class A> void kslices(A& a, long wgs) {
    long splits = wgs / a.tiles();
    if (splits < 1) splits = 1;
    if (splits > a.total) splits = a.total;
    a.sps = (int)((a.total + splits - 1) / splits);
    a.splits = (a.total + a.sps - 1) / a.sps;
}

// Where the n planned problems of a batch sit in the contraction launch (wg0), the reduce launch (tile0) and the workspace (ws;
// workspace may be null when only the sizes are wanted).  xcd_map(a, first workgroup) is the kind's rule for a.xcd_map.
struct BatchLayout {
    int wgs = 0, red_tiles = 0, max_splits = 1;      // workgroups, tiles of the problems that have k-slices, their most k-slices
    size_t ws_floats = 0;
};
template <class A, class X> BatchLayout batch_layout(int n, A* p, void* workspace, X xcd_map) {
    BatchLayout L;
    for (int i = 0; i < n; ++i) {
        A& a = p[i];
        a.ws = workspace ? (float*)workspace + L.ws_floats : nullptr;
        a.xcd_map = xcd_map(a, L.wgs);
        a.wg0 = L.wgs; L.wgs += a.tiles() * a.splits;
        a.tile0 = L.red_tiles;
        if (a.splits > 1) { L.red_tiles += a.tiles(); L.ws_floats += (size_t)a.splits * a.tiles() * a.tile_floats(); }
        if (a.splits > L.max_splits) L.max_splits = a.splits;
    }
    return L;
}
// What a batched entry point requires of the workspace it is handed
inline bool ws_ok(size_t ws_floats, const void* workspace, size_t ws_bytes) {
    return ws_floats == 0 || (workspace && ((uintptr_t)workspace & 15) == 0 && ws_bytes >= ws_floats * sizeof(float));
}

// The problem of a batch that workgroup `wg` of the contraction launch / tile `tile` of the reduce launch belongs to
template <class B> __device__ __forceinline__ int batch_problem(const B& b, int wg) {
    int p = 0;
#pragma unroll
    for (int q = 1; q < MAXP; ++q)
        if (q < b.n && wg >= b.p[q].wg0) p = q;
    return p;
}
template <class B> __device__ __forceinline__ int reduce_problem(const B& b, int tile) {
    int p = 0;
#pragma unroll
    for (int q = 1; q < MAXP; ++q)
        if (q < b.n && b.p[q].splits > 1 && tile >= b.p[q].tile0) p = q;
    return p;
}

// Consecutive workgroup ids go to different XCDs (id % 8), each with its own L2, and the tiles of one k-slice read the same rows: rank
// the W workgroups of a problem that starts at wg0 by (XCD, order on that XCD), and hand out (k-slice, tile) in rank order -- a slice's
// tiles then sit on one XCD and its rows come from HBM once.  Any wg0 and W; wg = workgroup within the problem.
__device__ __forceinline__ int xcd_rank(int wg0, int W, int wg) {
    const int x = (wg0 + wg) & 7;
    int rank = (wg - ((x - wg0) & 7)) >> 3;
    for (int xx = 0; xx < x; ++xx) rank += (W - ((xx - wg0) & 7) + 7) >> 3;
    return rank;
}

// One element of dW: added to, or (MI_WGRAD_STORE) written -- the element has no other writer in the call
__device__ __forceinline__ void wg_put(float* e, float v, int store) {
    if (store) *e = v;
    else *e += v;
}

// The reduce kernels: 256 threads = G slice groups x IB = 256 / G float4 positions.  p = this thread's position in k-slice 0 of its
// tile, `stride` floats from slice to slice.  Group g sums slices g, g + G, ... with 8 independent 16-byte loads in flight, the groups
// are folded through LDS in group order (every order here is fixed: the sum is deterministic), and the threads of group 0 hand
// the total to put(total), the kernel's placement into dW; the others are done.  Every thread of the workgroup must call (barrier).
// The slices behind the 8-wide loop are added one by one (TAIL_TOGETHER = false) or requested together, up to seven of them
// (true) -- the two add in different orders, and each kernel keeps its own.
template <int G, bool TAIL_TOGETHER, class Put>
__device__ __forceinline__ void slice_sum(const float* p, size_t stride, int splits, Put&& put) {
    constexpr int IB = 256 / G;
    __shared__ f32x4 red[G][IB];
    const int it = threadIdx.x % IB, grp = threadIdx.x / IB;
    f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0, s2 = s0, s3 = s0;
    int sp = grp;
    for (; sp + 7 * G < splits; sp += 8 * G) {
        f32x4 v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = *reinterpret_cast<const f32x4*>(p + (size_t)(sp + q * G) * stride);
        s0 += v[0] + v[4]; s1 += v[1] + v[5]; s2 += v[2] + v[6]; s3 += v[3] + v[7];
    }
    if constexpr (TAIL_TOGETHER) {
        f32x4 v[7];
#pragma unroll
        for (int q = 0; q < 7; ++q) v[q] = (sp + q * G < splits) ? *reinterpret_cast<const f32x4*>(p + (size_t)(sp + q * G) * stride) : f32x4{0.f, 0.f, 0.f, 0.f};
        s0 += v[0] + v[4]; s1 += v[1] + v[5]; s2 += v[2] + v[6]; s3 += v[3];
    } else {
        for (; sp < splits; sp += G) s0 += *reinterpret_cast<const f32x4*>(p + (size_t)sp * stride);
    }
    f32x4 s = (s0 + s1) + (s2 + s3);
    red[grp][it] = s;
    __syncthreads();
    if (grp != 0) return;
#pragma unroll
    for (int g = 1; g < G; ++g) s += red[g][it];
    put(s);
}

// LDS-DMA: 16 bytes per lane from each lane's own global address to LDS byte address lds_dst (wave-uniform) + 16 * lane.
// M0 carries the LDS base and is compiler-reserved: it is saved, set and restored inside the one statement.  The compiler does
// not know this is a load: completion is waited for with explicit s_waitcnt vmcnt(N) below.
__device__ __forceinline__ void glds16(const void* gsrc, uint32_t lds_dst) {
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}

__device__ __forceinline__ bf16x8 tr_pair(uint32_t a0, uint32_t a1) {
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(uintptr_t)a0);
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(uintptr_t)a1);
    const s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8, v);
}

}  // namespace
