// More than one EM iteration of the Wiener filter (norbert/__init__.py:133-148, the loop `for it in range(iterations)`
// of expectation_maximization; :247-260, wiener: ONE scaling by max(1, 0.1 max|x|) around all iterations).  The
// arithmetic is that of wiener_math.h.
//
// Two forms.
//   looped    iteration 1 is the three launches of wiener.hip; every further iteration is k_wiener_stats<YFrom::Current> (raw sums of
//             the CURRENT estimates, which wiener.hip keeps in unscaled units, and R from them with the 1/ma^2 the first
//             finalize left in the stats slot: the scale is carried there, Y is never rescaled and never divided twice)
//             followed by k_wiener_apply in place.  Any window length.  Per time-frequency point and extra iteration:
//             64 B (statistics) + 80 B read + 64 B written (apply) = 208 B.
//   resident  k_wiener_resident: one workgroup per (row, window) holds the window's frames in registers over all
//             iterations -- one read of the mix and the masks (or the initial estimates), one write of the estimates,
//             whatever niter is.  After the first iteration y_j[n] = v_j[n] R_j z[n] with z = Cxx^-1 x, so a frame is
//             carried by x (4 floats) and the four v_j (4 floats); the 16 floats of y exist only while a frame's sums are
//             taken and at the final store.  1024 threads x 5 frames = windows of up to 5120 frames; 40 registers of state
//             per thread, one workgroup (16 waves) per CU at <= 128 registers.  The 16 sums of an iteration are reduced
//             by a wave butterfly and a fixed-order tree over the 16 wave partials in LDS: no atomics, bitwise
//             reproducible.  The window maximum (shared over the rows of a batch group) comes from a pass over x alone,
//             k_wiener_window_max.  Per point: 16 B (maximum) + 48 B read (masked; 80 B from estimates) + 64 B written.
#pragma once
#include "wiener_math.h"

namespace xsq {

static constexpr int RES_THREADS = 1024;
static constexpr int RES_WAVES = RES_THREADS / 64;
// frames per thread: a frame between iterations is x (4 floats) and the J values v_j -- 8 * 5 = 40 floats of state and 16 sums at
// J = 4.  At J = 5 five frames are 45 floats and 20 sums: the gfx950 build then spills (128 VGPRs + 12 spilled, 32 B of scratch per
// lane), so that instantiation holds four (36 floats; 120 VGPRs, no scratch) and `auto` takes the looped form for windows above
// 4096 frames.  DESIGN.md 4.10 has the figures of every instantiation.
template <int J> struct Res;
template <> struct Res<4> { static constexpr int FPT = 5; };
template <> struct Res<5> { static constexpr int FPT = 4; };
template <int J> static constexpr int res_max_window = RES_THREADS * Res<J>::FPT;      // J = 4: 5120 >= the default window of 5000 frames

// ---- window-resident form ---------------------------------------------------------------------------------------------
// the workgroup's 4J sums, the same bits in every thread
template <int NV>
__device__ inline void res_reduce(float (&acc)[NV], float (*red)[NV], float* tot) {
    reduce<RES_WAVES>(acc, red, tot);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) acc[i] = tot[i];
    // (the next write of `red` comes after the second barrier, the next write of `tot` after the next call's first barrier:
    //  every thread has read what it needs by then)
}

// sums taken in scaled units -> R
template <int J>
__device__ inline void res_R(const float (&s)[4 * J], WR<J>& R) {
#pragma unroll
    for (int j = 0; j < J; ++j) {
        float den;
        sums_to_R(s[4 * j], s[4 * j + 1], s[4 * j + 2], s[4 * j + 3], 1.f, R.r00[j], R.r11[j], R.r01[j], den);
    }
}

// MASKED: the initial estimates come from the masks and the mix (Mk: real arena of 8B channels; start_channel: mask * x, the
// residual and the softmask as the frame is loaded), else they are Y itself (2JB channels; read before it is overwritten: each
// thread reads and writes only its own frames).  wmax / ext_max: max |x|^2 per (block, group, window) in blockwin order.
template <bool MASKED, int J, Start ST>
__global__ __launch_bounds__(RES_THREADS) void k_wiener_resident(const float2* __restrict__ X, const float* __restrict__ Mk,
                                                                  float2* Y, const WRow* __restrict__ rows,
                                                                  const int* __restrict__ work, const int* __restrict__ bw_of_work,
                                                                  const float* __restrict__ wmax, const float* __restrict__ ext_max,
                                                                  int Bn, int S, int win_len, int niter) {
    constexpr int FPT = Res<J>::FPT, NV = 4 * J;
    __shared__ float red[RES_WAVES][NV];
    __shared__ float tot[NV];
    const int row = work[2 * blockIdx.x], w = work[2 * blockIdx.x + 1];
    const WRow r = rows[row];
    const WWin W = window_of(r, S, w, win_len);                          // n1 - n0 <= res_max_window<J> (checked by the host)
    const int64_t N = W.N, n0 = W.n0, n1 = W.n1;
    const int bw = bw_of_work[blockIdx.x];
    const float mx2 = ext_max ? fmaxf(wmax[bw], ext_max[bw]) : wmax[bw];
    const float ma = fmaxf(1.f, 0.1f * sqrtf(mx2));                      // norbert :257
    const float inv_ma = 1.f / ma;
    const float2* x0p = X + aidx(r, 2 * Bn, S, r.b * 2, 0);
    const float2* x1p = X + aidx(r, 2 * Bn, S, r.b * 2 + 1, 0);
    const int64_t cstride = (int64_t)r.F * N, jstride = (int64_t)Bn * 2 * cstride;
    const float* m00 = Mk + aidx(r, 8 * Bn, S, r.b * 2, 0);              // target 0, channel 0 of this row in the masks' arena
    float2* y00 = Y + aidx(r, 2 * J * Bn, S, r.b * 2, 0);                // and in the estimates' (the same index at J = 4)

    // a frame between iterations: the scaled mix x' = x / ma and the J values v_j of the current estimates
    float2 xs0[FPT], xs1[FPT];
    float v[FPT][J];
    float acc[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) acc[i] = 0.f;
#pragma unroll
    for (int k = 0; k < FPT; ++k) {
        const int64_t n = n0 + k * RES_THREADS + threadIdx.x;
        xs0[k] = xs1[k] = make_float2(0.f, 0.f);
#pragma unroll
        for (int j = 0; j < J; ++j) v[k][j] = 0.f;
        if (n < n1) {
            const float2 a = x0p[n], b = x1p[n];
            xs0[k] = make_float2(a.x * inv_ma, a.y * inv_ma);
            xs1[k] = make_float2(b.x * inv_ma, b.y * inv_ma);
            float2 s0[J], s1[J];
            if constexpr (MASKED) {
                float m0[4], m1[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) { m0[j] = m00[j * jstride + n]; m1[j] = m00[j * jstride + cstride + n]; }
                start_channel<J, ST, true>(a, m0, s0);                   // J = 4, MixPhase: the products the layer-4 epilogue would have stored
                start_channel<J, ST, true>(b, m1, s1);
            }
#pragma unroll
            for (int j = 0; j < J; ++j) {
                float2 y0, y1;
                if constexpr (MASKED) {
                    y0 = s0[j];
                    y1 = s1[j];
                } else {
                    y0 = y00[j * jstride + n];
                    y1 = y00[j * jstride + cstride + n];
                }
                y0 = make_float2(y0.x * inv_ma, y0.y * inv_ma);
                y1 = make_float2(y1.x * inv_ma, y1.y * inv_ma);
                accumulate(acc, j, y0, y1);
                v[k][j] = power(y0, y1, 1.f);
            }
        }
    }
    res_reduce(acc, red, tot);

    WR<J> R;
    for (int it = 1; it < niter; ++it) {                                 // iterations 1 .. niter - 1: new v and new sums
        res_R<J>(acc, R);
#pragma unroll
        for (int i = 0; i < NV; ++i) acc[i] = 0.f;
#pragma unroll
        for (int k = 0; k < FPT; ++k) {
            if (n0 + k * RES_THREADS >= n1) break;                       // uniform over the workgroup
            float2 z0, z1;
            solve(invert_cxx(R, v[k]), xs0[k], xs1[k], z0, z1);         // (a frame past n1 has x = 0, v = 0: y = 0, adds nothing)
#pragma unroll
            for (int j = 0; j < J; ++j) {
                float2 y0, y1;
                source(R, j, v[k][j], z0, z1, y0, y1);
                accumulate(acc, j, y0, y1);
                v[k][j] = power(y0, y1, 1.f);
            }
        }
        res_reduce(acc, red, tot);
    }
    res_R<J>(acc, R);                                                     // the last iteration: the estimates, times ma
#pragma unroll
    for (int k = 0; k < FPT; ++k) {
        const int64_t n = n0 + k * RES_THREADS + threadIdx.x;
        if (n < n1) {
            float2 z0, z1;
            solve(invert_cxx(R, v[k]), xs0[k], xs1[k], z0, z1);
#pragma unroll
            for (int j = 0; j < J; ++j) {
                float2 y0, y1;
                source(R, j, v[k][j], z0, z1, y0, y1);
                y00[j * jstride + n] = make_float2(ma * y0.x, ma * y0.y);
                y00[j * jstride + cstride + n] = make_float2(ma * y1.x, ma * y1.y);
            }
        }
    }
}

}  // namespace xsq
