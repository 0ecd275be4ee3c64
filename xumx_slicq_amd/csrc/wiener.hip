// Mix-phase estimate and norbert Wiener-EM on the coefficient arena, gfx950.
//
// Reference: xumx_slicq_v2/phase.py:18-69 (blockwise_wiener: windows of <= 5000 frames over the
// flattened (slice, time) axis), :96-113 (blockwise_phasemix_sep); norbert/__init__.py:153-260
// (wiener, iterations=1, use_softmask=False) -> expectation_maximization :10-150 ->
// get_local_gaussian_model :458-494, get_mix_model :416-437, _invert :312-350,
// wiener_gain :353-388, apply_filter :391-413.
//
// Per (block, window w, batch item b, bin f) with frames n in the window, channels c,d in {0,1},
// sources j in {0..3}, y0 = initial estimate (mask * X), ma = max(1, 0.1 * max |x|) over the whole
// window INCLUDING the batch dimension (norbert :257), y' = y0/ma, x' = x/ma:
//   v'[n,j]  = mean_c |y'[n,c,j]|^2
//   R[j]     = sum_n y'[n,:,j] y'[n,:,j]^H / (sum_n v'[n,j] + eps)          eps = FLT_EPSILON
//   Cxx[n]   = sum_j v'[n,j] R[j] + sqrt(eps) I ;  y[n,:,j] = ma * v'[n,j] R[j] Cxx[n]^-1 x'[n]
// Three launches: k_wiener_stats (raw sums + max per row/window, fixed-order LDS tree, no atomics
// -> bitwise reproducible), k_wiener_finalize (window max, R), k_wiener_apply (elementwise 2x2
// solve, in place on Y).  All reads/writes are contiguous along the frame axis.
//
// The arithmetic is written once, in wiener_math.h: the sums of a frame, the workgroup reduction, sums -> R, Cxx^-1 and
// y_j = v_j R_j z.  The kernels here differ in where the estimates come from and where the results go:
//   k_wiener_stats<YFrom>    Estimates: the arena Y | Masks: mask * mix, formed on the way in | Current: Y again, in a later
//                            iteration (no maximum; R straight from the sums with the 1/ma^2 of iteration 1)
//   k_wiener_apply[_masked]  one / two frames per thread through wiener_point
//   k_wiener_bwd_*           the backward of one iteration (training)
//   k_wiener_resident        all iterations of a window on chip (wiener_iter.h)
// and the host side has one path: check_em -> run_em (the three launches) / run_resident, then run_more_iterations.
//
// More iterations (niter of the Open-Unmix family; norbert/__init__.py:133-148 loops, :247-260 scales ONCE
// around the loop): xsq_wiener_em_iter / xsq_wiener_em_masked_iter below.  niter = 1 runs exactly the three
// launches above.  niter >= 2 runs either the looped form (iteration 1 as above, then per iteration the
// statistics of the current estimates and the apply kernel in place; any window length) or the
// window-resident form (one workgroup per (row, window) keeps the window's frames in registers over all
// iterations: one read, one write; windows of at most xsq_wiener_resident_max_window() frames) --
// wiener_iter.h.  `method` chooses: 0 = resident when the window fits, 1 = looped, 2 = resident.
//
// Option sets (softmask, residual; norbert/__init__.py:247-248, :263-309 and norbert/contrib.py:11-77): the source count J (4, or 5
// with the residual last) and the kind of start are template parameters of every kernel here and of the arithmetic in
// wiener_math.h (start_channel: the J initial estimates of a channel from the mix and the four masks or magnitudes, formed as a
// frame is loaded).  The estimates' arena then has 2JB channels and the statistics slot Slot<J>::N floats; the masks' arena keeps
// 8B.  k_wiener_start writes the starts alone (niter = 0, and xsq_wiener_start for callers that hold magnitudes).  The entry points
// without options run the <4, MixPhase> instantiations: the code and the launches they always ran.  xsq_wiener_*_options below.
#include <cfloat>
#include <cmath>
#include <type_traits>
#include <vector>

#include "../../include/xumx_slicq_hip.h"
#include "plan.h"
#include "prof.h"
#include "wiener_iter.h"
#include "wiener_math.h"

namespace xsq {

struct WTable {
    WRow* d_rows = nullptr;
    int* d_work = nullptr;     // (row, window) pairs for the stats / finalize launches
    int nrows = 0, nwork = 0, nblockwin = 0;
    int* d_blockwin = nullptr; // (first_row, window) per (block, window)
    int* d_bw_of_work = nullptr;   // per (row, window) work item: index of its (block, group, window) in d_blockwin order
    int64_t max_frames = 0;
};

static std::mutex g_wmu;
static std::map<std::vector<int>, WTable> g_wtables;

// ---- Y = mag * x/|x|  (phase.py:96-113; angle(0) = 0) --------------------------------------------
// (unit_phase: wiener_math.h)
__global__ __launch_bounds__(256) void k_phasemix(const float2* __restrict__ X, const float* __restrict__ mag,
                                                   float2* __restrict__ Y, const WRow* __restrict__ rows, int Bn,
                                                   int S) {
    const WRow r = rows[blockIdx.y];
    const int64_t N = (int64_t)S * r.T;
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const float2 x = X[aidx(r, 2 * Bn, S, r.b * 2 + c, n)];
        const float2 u = unit_phase(x);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t yi = aidx(r, 8 * Bn, S, (j * Bn + r.b) * 2 + c, n);
            const float m = mag[yi];
            Y[yi] = make_float2(m * u.x, m * u.y);
        }
    }
}

// ---- the J initial estimates under an option set (softmask, residual), into the estimates' arena of 2JB channels: the result of
// niter = 0 and what the forms fed by estimates start from.  a: the masks (MASKS) or the magnitudes, real arena of 8B channels.
template <int J, Start ST, bool MASKS>
__global__ __launch_bounds__(256) void k_wiener_start(const float2* __restrict__ X, const float* __restrict__ a,
                                                       float2* __restrict__ Y, const WRow* __restrict__ rows, int Bn, int S) {
    const WRow r = rows[blockIdx.y];
    const int64_t N = (int64_t)S * r.T;
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const float2 x = X[aidx(r, 2 * Bn, S, r.b * 2 + c, n)];
        float m[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) m[j] = a[aidx(r, 8 * Bn, S, (j * Bn + r.b) * 2 + c, n)];
        float2 y[J];
        start_channel<J, ST, MASKS>(x, m, y);
#pragma unroll
        for (int j = 0; j < J; ++j) Y[aidx(r, 2 * J * Bn, S, (j * Bn + r.b) * 2 + c, n)] = y[j];
    }
}

// ---- pass 1: raw sums and max per (row, window).  One workgroup per (row, window). -----------------
// Lane t adds frames n0 + t, n0 + t + 256, ... in order, whatever the source: the sums round identically.
//   Estimates  y = Y[n]: 80 B per time-frequency point.
//   Masks      y = mask * x, the products the CDAE's layer-4 epilogue would have stored (one fp32 rounding each): the layer
//              then writes 4 bytes per coefficient instead of 8 and this pass reads 48 B.  Bitwise the two-step result.
//   Current    y = Y[n] in iterations >= 2 of the looped form.  st[16] holds 1/ma^2 (k_wiener_finalize of iteration 1) and is
//              left alone; st[0..15] become R, st[20..23] the denominators: the arithmetic of k_wiener_finalize.
// J sources (Slot<J>: the slot above is J = 4) and, from masks, the kind of start (start_channel: the residual and the softmask
// are formed on the way in; J = 4 from the mixture phase is the line above).
//   Sources    the oracle (slicqfinder.py): Y holds the coefficients of the four true sources; the mix, its maximum and the
//              starts |s_j| m/|m| are formed on the way in (sources_channel).  64 B per point, X is not read.
enum class YFrom { Estimates, Masks, Current, Sources };

template <YFrom SRC, int J, Start ST>
__global__ __launch_bounds__(256) void k_wiener_stats(const float2* __restrict__ X, const float2* __restrict__ Y,
                                                       const float* __restrict__ Mk, const WRow* __restrict__ rows,
                                                       const int* __restrict__ work, float* __restrict__ stats, int Bn, int S,
                                                       int win_len) {
    constexpr bool MAX = SRC != YFrom::Current;
    constexpr int NV = MAX ? 4 * J + 1 : 4 * J;
    const int row = work[2 * blockIdx.x], w = work[2 * blockIdx.x + 1];
    const WRow r = rows[row];
    const WWin W = window_of(r, S, w, win_len);
    float acc[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) acc[i] = 0.f;
    const float2* x0 = SRC == YFrom::Sources ? nullptr : X + aidx(r, 2 * Bn, S, r.b * 2, 0);
    const float2* x1 = SRC == YFrom::Sources ? nullptr : X + aidx(r, 2 * Bn, S, r.b * 2 + 1, 0);
    // target 0, channel 0 of this row: in the masks' arena (8B channels) or the estimates' (2JB); the same index at J = 4
    const int64_t base = aidx(r, SRC == YFrom::Masks ? 8 * Bn : 2 * J * Bn, S, r.b * 2, 0);
    const int64_t cstride = (int64_t)r.F * W.N, jstride = (int64_t)Bn * 2 * cstride;
    for (int64_t n = W.n0 + threadIdx.x; n < W.n1; n += 256) {
        float2 a, b;
        if constexpr (MAX && SRC != YFrom::Sources) {
            a = x0[n], b = x1[n];
            acc[NV - 1] = fmaxf(acc[NV - 1], fmaxf(abs2(a), abs2(b)));
        }
        if constexpr (SRC == YFrom::Sources) {
            static_assert(J == 4, "the oracle has the four targets");
            float2 s0[4], s1[4], y0[4], y1[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) { s0[j] = Y[base + j * jstride + n]; s1[j] = Y[base + j * jstride + cstride + n]; }
            sources_channel(s0, a, y0);
            sources_channel(s1, b, y1);
            acc[NV - 1] = fmaxf(acc[NV - 1], fmaxf(abs2(a), abs2(b)));
#pragma unroll
            for (int j = 0; j < 4; ++j) accumulate(acc, j, y0[j], y1[j]);
        } else if constexpr (SRC == YFrom::Masks && (J != 4 || ST != Start::MixPhase)) {
            float m0[4], m1[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) { m0[j] = Mk[base + j * jstride + n]; m1[j] = Mk[base + j * jstride + cstride + n]; }
            float2 y0[J], y1[J];
            start_channel<J, ST, true>(a, m0, y0);
            start_channel<J, ST, true>(b, m1, y1);
#pragma unroll
            for (int j = 0; j < J; ++j) accumulate(acc, j, y0[j], y1[j]);
        } else {
#pragma unroll
            for (int j = 0; j < J; ++j) {
                const int64_t i = base + j * jstride + n;
                if constexpr (SRC == YFrom::Masks) {
                    const float ma = Mk[i], mb = Mk[i + cstride];
                    accumulate(acc, j, make_float2(ma * a.x, ma * a.y), make_float2(mb * b.x, mb * b.y));
                } else {
                    accumulate(acc, j, Y[i], Y[i + cstride]);
                }
            }
        }
    }
    __shared__ float red[4][NV];
    float* st = stats + r.stat + (int64_t)w * Slot<J>::N;
    if constexpr (MAX) {
        reduce<4>(acc, red, st);
    } else {
        __shared__ float tot[4 * J];
        reduce<4>(acc, red, tot);
        __syncthreads();
        if (threadIdx.x < J) sums_to_R_slot<J>(st, threadIdx.x, tot, st[Slot<J>::MAX]);
    }
}

// ---- pass 2: window max over all rows of the block, then R per row.  One workgroup per (block, window).
// ext_max (optional): max |x|^2 per (block, group, window) in blockwin order, taken over MORE batch items than this call holds
// (a batch split into several passes, demix.hip): the window maximum of norbert :257 spans the whole batch.
template <int J>
__global__ __launch_bounds__(256) void k_wiener_finalize(const WRow* __restrict__ rows,
                                                          const int* __restrict__ blockwin,
                                                          float* __restrict__ stats, const float* __restrict__ ext_max) {
    const int first = blockwin[2 * blockIdx.x], w = blockwin[2 * blockIdx.x + 1];
    const int nrows = rows[first].nrows;
    __shared__ float smax[256];
    float m = 0.f;
    for (int i = threadIdx.x; i < nrows; i += 256) m = fmaxf(m, stats[rows[first + i].stat + (int64_t)w * Slot<J>::N + Slot<J>::MAX]);
    smax[threadIdx.x] = m;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) smax[threadIdx.x] = fmaxf(smax[threadIdx.x], smax[threadIdx.x + s]);
        __syncthreads();
    }
    const float mx2 = ext_max ? fmaxf(smax[0], ext_max[blockIdx.x]) : smax[0];
    const float ma = fmaxf(1.f, 0.1f * sqrtf(mx2));         // norbert :257
    const float inv_ma2 = 1.f / (ma * ma);
    for (int i = threadIdx.x; i < nrows; i += 256) {
        float* st = stats + rows[first + i].stat + (int64_t)w * Slot<J>::N;
#pragma unroll
        for (int j = 0; j < J; ++j) sums_to_R_slot<J>(st, j, st, inv_ma2);
        st[Slot<J>::MAX] = inv_ma2;
    }
}

// ---- pass 3: per time-frequency point 2x2 solve and filter, in place on Y ---------------------------
template <int J>
__global__ __launch_bounds__(256) void k_wiener_apply(const float2* __restrict__ X, float2* __restrict__ Y,
                                                       const WRow* __restrict__ rows, const float* __restrict__ stats,
                                                       int Bn, int S, int win_len) {
    const WRow r = rows[blockIdx.y];
    const int64_t N = (int64_t)S * r.T;
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const float* st = stats + r.stat + (n / win_len) * Slot<J>::N;
    const float2 x0 = X[aidx(r, 2 * Bn, S, r.b * 2, n)];
    const float2 x1 = X[aidx(r, 2 * Bn, S, r.b * 2 + 1, n)];
    float2 y[J][2], o[J][2];
    int64_t yi[J];
#pragma unroll
    for (int j = 0; j < J; ++j) {
        yi[j] = aidx(r, 2 * J * Bn, S, (j * Bn + r.b) * 2, n);
        y[j][0] = Y[yi[j]];
        y[j][1] = Y[yi[j] + (int64_t)r.F * N];
    }
    wiener_point<J>(st, x0, x1, y, o);
#pragma unroll
    for (int j = 0; j < J; ++j) {
        Y[yi[j]] = o[j][0];
        Y[yi[j] + (int64_t)r.F * N] = o[j][1];
    }
}

// the starts of frame n (second = false) or n + 1 of the two-frame loads of k_wiener_apply_masked
template <int J, Start ST>
__device__ inline void point_start(float2 x0, float2 x1, const float2 (&ma)[4], const float2 (&mb)[4], bool second, float2 (&y)[J][2]) {
    float m0[4], m1[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { m0[j] = second ? ma[j].y : ma[j].x; m1[j] = second ? mb[j].y : mb[j].x; }
    float2 y0[J], y1[J];
    start_channel<J, ST, true>(x0, m0, y0);
    start_channel<J, ST, true>(x1, m1, y1);
#pragma unroll
    for (int j = 0; j < J; ++j) { y[j][0] = y0[j]; y[j][1] = y1[j]; }
}

// The same pass fed by masks: pass 3 reads 48 B and writes 64 B instead of 80 + 64.  Two frames per thread (N = S*T and the
// window length are even on this path): 16-byte loads of the mix, 8-byte loads of the masks, 16-byte stores.  J sources from the
// start ST (start_channel); the masks' arena has 8B channels, the estimates' 2JB.
template <int J, Start ST>
__global__ __launch_bounds__(256) void k_wiener_apply_masked(const float2* __restrict__ X, const float* __restrict__ Mk,
                                                              float2* __restrict__ Y, const WRow* __restrict__ rows,
                                                              const float* __restrict__ stats, int Bn, int S, int win_len) {
    const WRow r = rows[blockIdx.y];
    const int64_t N = (int64_t)S * r.T;
    const int64_t n = 2 * ((int64_t)blockIdx.x * 256 + threadIdx.x);       // frames n, n + 1 (same window: both even)
    if (n >= N) return;
    const float* st = stats + r.stat + (n / win_len) * Slot<J>::N;
    const float4 xa = *reinterpret_cast<const float4*>(X + aidx(r, 2 * Bn, S, r.b * 2, n));
    const float4 xb = *reinterpret_cast<const float4*>(X + aidx(r, 2 * Bn, S, r.b * 2 + 1, n));
    const int64_t cstride = (int64_t)r.F * N, jstride = (int64_t)Bn * 2 * cstride;
    const float* m0 = Mk + aidx(r, 8 * Bn, S, r.b * 2, n);
    float2 ma[4], mb[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        ma[j] = *reinterpret_cast<const float2*>(m0 + j * jstride);
        mb[j] = *reinterpret_cast<const float2*>(m0 + j * jstride + cstride);
    }
    float2 y[J][2], o0[J][2], o1[J][2];
    if constexpr (J == 4 && ST == Start::MixPhase) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            y[j][0] = make_float2(ma[j].x * xa.x, ma[j].x * xa.y);
            y[j][1] = make_float2(mb[j].x * xb.x, mb[j].x * xb.y);
        }
    } else {
        point_start<J, ST>(make_float2(xa.x, xa.y), make_float2(xb.x, xb.y), ma, mb, false, y);
    }
    wiener_point<J>(st, make_float2(xa.x, xa.y), make_float2(xb.x, xb.y), y, o0);
    if constexpr (J == 4 && ST == Start::MixPhase) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            y[j][0] = make_float2(ma[j].y * xa.z, ma[j].y * xa.w);
            y[j][1] = make_float2(mb[j].y * xb.z, mb[j].y * xb.w);
        }
    } else {
        point_start<J, ST>(make_float2(xa.z, xa.w), make_float2(xb.z, xb.w), ma, mb, true, y);
    }
    wiener_point<J>(st, make_float2(xa.z, xa.w), make_float2(xb.z, xb.w), y, o1);
    float2* y0p = Y + aidx(r, 2 * J * Bn, S, r.b * 2, n);
#pragma unroll
    for (int j = 0; j < J; ++j) {
        *reinterpret_cast<float4*>(y0p + j * jstride) = make_float4(o0[j][0].x, o0[j][0].y, o1[j][0].x, o1[j][0].y);
        *reinterpret_cast<float4*>(y0p + j * jstride + cstride) = make_float4(o0[j][1].x, o0[j][1].y, o1[j][1].x, o1[j][1].y);
    }
}

// The same pass fed by the sources' coefficients (the oracle): Sc and Y are arenas of 8B complex channels, 64 B read and 64 B
// written per point, and Y == Sc is allowed -- a thread reads its frames of all eight channels before it stores any, and no other
// thread touches them (no __restrict__ on the two).  EM = false stops at the starts |s_j| m/|m| (xsq_phasemix_sources: no
// statistics, no window).  A thread owns the frames n, n + 1: one 16-byte access per channel where the row allows it (S*T even;
// with EM an even window too, so that both frames share a slot), else 8-byte accesses frame by frame -- the arithmetic of a
// frame is the same either way.
template <bool EM>
__device__ inline void sources_point(const float* __restrict__ st, const float2 (&s)[4][2], float2 (&o)[4][2]) {
    float2 s0[4], s1[4], y0[4], y1[4], m0, m1;
#pragma unroll
    for (int j = 0; j < 4; ++j) { s0[j] = s[j][0]; s1[j] = s[j][1]; }
    sources_channel(s0, m0, y0);
    sources_channel(s1, m1, y1);
    float2 y[4][2];
#pragma unroll
    for (int j = 0; j < 4; ++j) { y[j][0] = y0[j]; y[j][1] = y1[j]; }
    if constexpr (EM) {
        wiener_point<4>(st, m0, m1, y, o);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) { o[j][0] = y[j][0]; o[j][1] = y[j][1]; }
    }
}

template <bool EM>
__global__ __launch_bounds__(256) void k_wiener_apply_sources(const float2* Sc, float2* Y, const WRow* __restrict__ rows,
                                                               const float* __restrict__ stats, int Bn, int S, int win_len) {
    const WRow r = rows[blockIdx.y];
    const int64_t N = (int64_t)S * r.T;
    const int64_t n = 2 * ((int64_t)blockIdx.x * 256 + threadIdx.x);
    if (n >= N) return;
    const int64_t cstride = (int64_t)r.F * N, jstride = (int64_t)Bn * 2 * cstride;
    const int64_t i0 = aidx(r, 8 * Bn, S, r.b * 2, n);
    const bool wide = N % 2 == 0 && (!EM || win_len % 2 == 0);          // the same for every thread of the row
    float2 s[4][2], o[4][2];
    if (wide) {
        const float* st = EM ? stats + r.stat + (n / win_len) * Slot<4>::N : nullptr;
        float4 in[4][2];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            in[j][0] = *reinterpret_cast<const float4*>(Sc + i0 + j * jstride);
            in[j][1] = *reinterpret_cast<const float4*>(Sc + i0 + j * jstride + cstride);
        }
        float2 o1[4][2];
#pragma unroll
        for (int j = 0; j < 4; ++j) { s[j][0] = make_float2(in[j][0].x, in[j][0].y); s[j][1] = make_float2(in[j][1].x, in[j][1].y); }
        sources_point<EM>(st, s, o);
#pragma unroll
        for (int j = 0; j < 4; ++j) { s[j][0] = make_float2(in[j][0].z, in[j][0].w); s[j][1] = make_float2(in[j][1].z, in[j][1].w); }
        sources_point<EM>(st, s, o1);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            *reinterpret_cast<float4*>(Y + i0 + j * jstride) = make_float4(o[j][0].x, o[j][0].y, o1[j][0].x, o1[j][0].y);
            *reinterpret_cast<float4*>(Y + i0 + j * jstride + cstride) = make_float4(o[j][1].x, o[j][1].y, o1[j][1].x, o1[j][1].y);
        }
        return;
    }
    for (int64_t k = n; k < n + 2 && k < N; ++k) {
        const float* st = EM ? stats + r.stat + (k / win_len) * Slot<4>::N : nullptr;
        const int64_t i = i0 + (k - n);
#pragma unroll
        for (int j = 0; j < 4; ++j) { s[j][0] = Sc[i + j * jstride]; s[j][1] = Sc[i + j * jstride + cstride]; }
        sources_point<EM>(st, s, o);
#pragma unroll
        for (int j = 0; j < 4; ++j) { Y[i + j * jstride] = o[j][0]; Y[i + j * jstride + cstride] = o[j][1]; }
    }
}

// ---- backward of the EM iteration (training: loss.backward() through norbert, training.py:107) --------
// Notation of the header; per point n: w = Cxx^-1 x, out_j = v_j R_j w.  With gO_j the incoming gradient,
//   q = sum_j v_j R_j gO_j,  p = Cxx^-1 q,  u_j = gO_j - p,
//   d/dv_j = Re(u_j^H R_j w),   d/dR_j = sum_n v_j u_j w^H  (only its Hermitian part K_j matters),
//   R_j = A_j / D_j:  H_j = K_j / D_j - Re tr(K_j/2 R_j) / D_j * I,
//   d/dy0[n,:,j] = (d/dv_j * y0 + H_j y0) / ma^2.
// Pass 1 accumulates K_j per (row, window) (same fixed-order reduction as the forward statistics), pass 2
// forms H_j, pass 3 rewrites the gradient arena in place.
struct WPoint {
    float v[4], gv[4];
    float2 u[4][2];
    float2 w0, w1;
};


__device__ inline void wiener_bwd_point(const float* __restrict__ st, float2 x0, float2 x1, const float2 (&y)[4][2],
                                        const float2 (&g)[4][2], WPoint& P) {
    const float inv_ma2 = st[16];
    WR<4> R;
    load_R(st, R);
#pragma unroll
    for (int j = 0; j < 4; ++j) P.v[j] = power(y[j][0], y[j][1], inv_ma2);
    const WInv I = invert_cxx(R, P.v);
    // Cxx^-1 a with i10 written as conj(i01): the same values as solve() of the forward pass with one multiply fewer; kept
    // so that the backward kernels' instructions stay what they were
    auto solve = [&](float2 a0, float2 a1, float2& o0, float2& o1) {
        const float2 t = cmul(I.i01, a1), s = cmulc(a0, I.i01);
        o0 = make_float2(I.i00 * a0.x + t.x, I.i00 * a0.y + t.y);
        o1 = make_float2(s.x + I.i11 * a1.x, s.y + I.i11 * a1.y);
    };
    solve(x0, x1, P.w0, P.w1);
    float2 q0 = make_float2(0.f, 0.f), q1 = q0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {       // v_j R_j gO_j
        float2 a, b;
        source(R, j, P.v[j], g[j][0], g[j][1], a, b);
        q0.x += a.x; q0.y += a.y;
        q1.x += b.x; q1.y += b.y;
    }
    float2 p0, p1;
    solve(q0, q1, p0, p1);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        P.u[j][0] = make_float2(g[j][0].x - p0.x, g[j][0].y - p0.y);
        P.u[j][1] = make_float2(g[j][1].x - p1.x, g[j][1].y - p1.y);
        float2 rw0, rw1;
        mul_R(R, j, P.w0, P.w1, rw0, rw1);
        P.gv[j] = (P.u[j][0].x * rw0.x + P.u[j][0].y * rw0.y) + (P.u[j][1].x * rw1.x + P.u[j][1].y * rw1.y);
    }
}

// Mk != nullptr: the pre-filter estimate is mask * x (the products the layer-4 epilogue would have stored)
__device__ inline void wiener_load_point(const float2* __restrict__ X, const float2* __restrict__ Y0, const float* __restrict__ Mk,
                                         const float2* __restrict__ G, const WRow& r, int Bn, int S, int64_t n,
                                         float2& x0, float2& x1, float2 (&y)[4][2], float2 (&g)[4][2], int64_t (&yi)[4]) {
    const int64_t N = (int64_t)S * r.T;
    x0 = X[aidx(r, 2 * Bn, S, r.b * 2, n)];
    x1 = X[aidx(r, 2 * Bn, S, r.b * 2 + 1, n)];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        yi[j] = aidx(r, 8 * Bn, S, (j * Bn + r.b) * 2, n);
        if (Mk) {
            const float ma = Mk[yi[j]], mb = Mk[yi[j] + (int64_t)r.F * N];      // real arena: same index, one float each
            y[j][0] = make_float2(ma * x0.x, ma * x0.y); y[j][1] = make_float2(mb * x1.x, mb * x1.y);
        } else {
            y[j][0] = Y0[yi[j]]; y[j][1] = Y0[yi[j] + (int64_t)r.F * N];
        }
        g[j][0] = G[yi[j]]; g[j][1] = G[yi[j] + (int64_t)r.F * N];
    }
}

__global__ __launch_bounds__(256) void k_wiener_bwd_stats(const float2* __restrict__ X, const float2* __restrict__ Y0,
                                                           const float* __restrict__ Mk,
                                                           const float2* __restrict__ G, const WRow* __restrict__ rows,
                                                           const int* __restrict__ work, const float* __restrict__ stats,
                                                           float* __restrict__ bstats, int Bn, int S, int win_len) {
    const int row = work[2 * blockIdx.x], w = work[2 * blockIdx.x + 1];
    const WRow r = rows[row];
    const WWin W = window_of(r, S, w, win_len);
    const float* st = stats + r.stat + (int64_t)w * STAT;
    float acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    for (int64_t n = W.n0 + threadIdx.x; n < W.n1; n += 256) {
        float2 x0, x1, y[4][2], g[4][2];
        int64_t yi[4];
        wiener_load_point(X, Y0, Mk, G, r, Bn, S, n, x0, x1, y, g, yi);
        WPoint P;
        wiener_bwd_point(st, x0, x1, y, g, P);
#pragma unroll
        for (int j = 0; j < 4; ++j) {      // K = v (u w^H + w u^H)
            const float2 a = cmulc(P.u[j][0], P.w1), b = cmulc(P.w0, P.u[j][1]);
            acc[4 * j + 0] += 2.f * P.v[j] * (P.u[j][0].x * P.w0.x + P.u[j][0].y * P.w0.y);
            acc[4 * j + 1] += 2.f * P.v[j] * (P.u[j][1].x * P.w1.x + P.u[j][1].y * P.w1.y);
            acc[4 * j + 2] += P.v[j] * (a.x + b.x);
            acc[4 * j + 3] += P.v[j] * (a.y + b.y);
        }
    }
    __shared__ float red[4][16];
    reduce<4>(acc, red, bstats + r.stat + (int64_t)w * STAT);
}

// K_j -> H_j, one thread per (row, window)
__global__ void k_wiener_bwd_finalize(const WRow* __restrict__ rows, const int* __restrict__ work, int nwork,
                                      const float* __restrict__ stats, float* __restrict__ bstats) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nwork) return;
    const WRow r = rows[work[2 * i]];
    const int64_t o = r.stat + (int64_t)work[2 * i + 1] * STAT;
    const float* st = stats + o;
    float* bs = bstats + o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float den = st[20 + j];
        const float k00 = bs[4 * j], k11 = bs[4 * j + 1], k01x = bs[4 * j + 2], k01y = bs[4 * j + 3];
        const float s = (0.5f * (k00 * st[4 * j] + k11 * st[4 * j + 1]) + (k01x * st[4 * j + 2] + k01y * st[4 * j + 3])) * den;
        bs[4 * j] = k00 * den - s;
        bs[4 * j + 1] = k11 * den - s;
        bs[4 * j + 2] = k01x * den;
        bs[4 * j + 3] = k01y * den;
    }
}

__global__ __launch_bounds__(256) void k_wiener_bwd_apply(const float2* __restrict__ X, const float2* __restrict__ Y0,
                                                           const float* __restrict__ Mk,
                                                           float2* __restrict__ G, const WRow* __restrict__ rows,
                                                           const float* __restrict__ stats, const float* __restrict__ bstats,
                                                           int Bn, int S, int win_len, float* __restrict__ gM = nullptr) {
    const WRow r = rows[blockIdx.y];
    const int64_t N = (int64_t)S * r.T;
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const int64_t o = r.stat + (n / win_len) * STAT;
    const float* st = stats + o;
    const float* bs = bstats + o;
    float2 x0, x1, y[4][2], g[4][2];
    int64_t yi[4];
    wiener_load_point(X, Y0, Mk, G, r, Bn, S, n, x0, x1, y, g, yi);
    WPoint P;
    wiener_bwd_point(st, x0, x1, y, g, P);
    const float inv_ma2 = st[16];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float h00 = bs[4 * j], h11 = bs[4 * j + 1];
        const float2 h01 = make_float2(bs[4 * j + 2], bs[4 * j + 3]);
        const float2 a = cmul(h01, y[j][1]), b = cmulc(y[j][0], h01);
        const float2 g0 = make_float2((P.gv[j] * y[j][0].x + h00 * y[j][0].x + a.x) * inv_ma2,
                                      (P.gv[j] * y[j][0].y + h00 * y[j][0].y + a.y) * inv_ma2);
        const float2 g1 = make_float2((P.gv[j] * y[j][1].x + b.x + h11 * y[j][1].x) * inv_ma2,
                                      (P.gv[j] * y[j][1].y + b.y + h11 * y[j][1].y) * inv_ma2);
        const int64_t i0 = yi[j], i1 = yi[j] + (int64_t)r.F * N;
        if (gM) {
            // training step: the gradient of the pre-filter estimate y0 = m x goes straight on through the product and the
            // sigmoid (train.hip: k_mask_bwd) -- d/dm = Re(conj(x) g) on top of the mask-sum gradient already in gM, times
            // m (1 - m) -- instead of being stored (64 B per point) and read back by a second pass
            const float m0 = Mk[i0], m1 = Mk[i1];
            gM[i0] = (x0.x * g0.x + x0.y * g0.y + gM[i0]) * m0 * (1.f - m0);
            gM[i1] = (x1.x * g1.x + x1.y * g1.y + gM[i1]) * m1 * (1.f - m1);
        } else {
            G[i0] = g0;
            G[i1] = g1;
        }
    }
}

// ---- max |x|^2 per (block, group, window) of ONE pass of a split batch, folded into ext_max (non-negative floats order
// like their bit patterns: atomicMax on the words).  One workgroup per (row, window), as the statistics pass.
__global__ __launch_bounds__(256) void k_wiener_window_max(const float2* __restrict__ X, const WRow* __restrict__ rows,
                                                            const int* __restrict__ work, const int* __restrict__ bw_of_work,
                                                            float* __restrict__ ext_max, int Bn, int S, int win_len) {
    const int row = work[2 * blockIdx.x], w = work[2 * blockIdx.x + 1];
    const WRow r = rows[row];
    const WWin W = window_of(r, S, w, win_len);
    const float2* x0 = X + aidx(r, 2 * Bn, S, r.b * 2, 0);
    const float2* x1 = X + aidx(r, 2 * Bn, S, r.b * 2 + 1, 0);
    float m = 0.f;
    for (int64_t n = W.n0 + threadIdx.x; n < W.n1; n += 256) m = fmaxf(m, fmaxf(abs2(x0[n]), abs2(x1[n])));   // as k_wiener_stats
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(reinterpret_cast<unsigned*>(ext_max) + bw_of_work[blockIdx.x], __builtin_bit_cast(unsigned, m));
}

// ------------------------------------------------------------------------------------------------
// slot: floats per (row, window) of the statistics (Slot<J>::N)
static int get_wtable(int nblocks, const int32_t* F, const int32_t* T, int Bn, int S, int win_len, int group, WTable* out, int slot = STAT) {
    std::vector<int> key;
    int dev = 0;
    XSQ_HIP(hipGetDevice(&dev));                 // the tables live in one device's memory: keyed by it
    key.push_back(dev);
    key.push_back(nblocks); key.push_back(Bn); key.push_back(S); key.push_back(win_len); key.push_back(group); key.push_back(slot);
    for (int b = 0; b < nblocks; ++b) { key.push_back(F[b]); key.push_back(T[b]); }
    std::lock_guard<std::mutex> lk(g_wmu);
    auto it = g_wtables.find(key);
    if (it != g_wtables.end()) { *out = it->second; return XSQ_OK; }
    std::vector<WRow> rows;
    std::vector<int> work, blockwin, bw_of_work;
    int64_t cum = 0, stat = 0, maxN = 0;
    for (int k = 0; k < nblocks; ++k) {
        const int64_t N = (int64_t)S * T[k];
        const int nwin = (int)((N + win_len - 1) / win_len);
        const int first = (int)rows.size();
        const int bw0 = (int)blockwin.size() / 2;          // this block's (group, window) entries start here
        maxN = N > maxN ? N : maxN;
        for (int b = 0; b < Bn; ++b)
            for (int f = 0; f < F[k]; ++f) {
                for (int w = 0; w < nwin; ++w) bw_of_work.push_back(bw0 + (b / group) * nwin + w);
                WRow r;
                r.F = F[k]; r.T = T[k]; r.b = b; r.f = f;
                r.nrows = group * F[k];      // rows sharing one window maximum: the `group` consecutive batch items of this row's group
                r.cum = cum; r.stat = stat;
                for (int w = 0; w < nwin; ++w) { work.push_back((int)rows.size()); work.push_back(w); }
                rows.push_back(r);
                stat += (int64_t)nwin * slot;
            }
        for (int gI = 0; gI < Bn / group; ++gI)
            for (int w = 0; w < nwin; ++w) { blockwin.push_back(first + gI * group * F[k]); blockwin.push_back(w); }
        cum += (int64_t)F[k] * T[k];
    }
    WTable t;
    t.nrows = (int)rows.size(); t.nwork = (int)work.size() / 2; t.nblockwin = (int)blockwin.size() / 2;
    t.max_frames = maxN;
    int rc = upload(t.d_rows, rows);
    if (!rc) rc = upload(t.d_work, work);
    if (!rc) rc = upload(t.d_blockwin, blockwin);
    if (!rc) rc = upload(t.d_bw_of_work, bw_of_work);
    if (rc) {       // not in the cache yet: nothing else would free what this call allocated
        (void)hipFree(t.d_rows); (void)hipFree(t.d_work); (void)hipFree(t.d_blockwin); (void)hipFree(t.d_bw_of_work);
        return rc;
    }
    g_wtables[key] = t;
    *out = t;
    return XSQ_OK;
}

static int check_table(const char* who, int nblocks, const int32_t* F, const int32_t* T, int Bn, int S) {
    XSQ_REQUIRE(nblocks > 0 && F && T, "%s: null block table", who);
    XSQ_REQUIRE(Bn > 0 && S > 0, "%s: B=%d S=%d", who, Bn, S);
    int64_t rows = 0;
    for (int b = 0; b < nblocks; ++b) {
        XSQ_REQUIRE(F[b] > 0 && T[b] > 0, "%s: block %d has F=%d T=%d", who, b, F[b], T[b]);
        rows += (int64_t)Bn * F[b];
    }
    XSQ_REQUIRE(rows <= 65535, "%s: %lld rows exceed one launch", who, (long long)rows);
    return XSQ_OK;
}

// backward of xsq_wiener_em: `stats` is the workspace the forward call left behind, G holds dL/d(out) on entry
// and dL/d(y0) on return, Y0 is the pre-filter estimate.  bstats: another workspace of the same size.
int wiener_em_backward(int nblocks, const int32_t* F, const int32_t* T, const float* X, const float* Y0, const float* masks,
                       float* G, int Bn, int S, int win_len, int batch_group, const void* stats, void* bstats, hipStream_t stream,
                       float* gM) {
    if (batch_group <= 0) batch_group = Bn;
    WTable t;
    int rc;
    if ((rc = get_wtable(nblocks, F, T, Bn, S, win_len, batch_group, &t))) return rc;
    { XSQ_PROF("wiener_bwd_stats", stream);
    hipLaunchKernelGGL(k_wiener_bwd_stats, dim3(t.nwork), dim3(256), 0, stream, (const float2*)X, (const float2*)Y0,
                       Y0 ? nullptr : masks, (const float2*)G, t.d_rows, t.d_work, (const float*)stats, (float*)bstats, Bn, S, win_len); }
    { XSQ_PROF("wiener_bwd_finalize", stream);
    hipLaunchKernelGGL(k_wiener_bwd_finalize, dim3((t.nwork + 255) / 256), dim3(256), 0, stream, t.d_rows, t.d_work, t.nwork,
                       (const float*)stats, (float*)bstats); }
    { XSQ_PROF("wiener_bwd_apply", stream);
    hipLaunchKernelGGL(k_wiener_bwd_apply, dim3((unsigned)((t.max_frames + 255) / 256), t.nrows), dim3(256), 0, stream,
                       (const float2*)X, (const float2*)Y0, Y0 ? nullptr : masks, (float2*)G, t.d_rows, (const float*)stats,
                       (const float*)bstats, Bn, S, win_len, (Y0 == nullptr && masks) ? gM : nullptr); }
    XSQ_HIP(hipGetLastError());
    return XSQ_OK;
}

// ---- forward: one path for every entry point ---------------------------------------------------------------------------
struct EmCall {                     // the arguments of a forward entry point
    int nblocks;
    const int32_t *F, *T;
    const float* X;
    const float* masks;             // the masked form (two frames per thread); nullptr: Y holds the initial estimates
    float* Y;
    int Bn, S, win_len, batch_group;
    const float* ext_max;
    void* ws;
    size_t ws_bytes;
    hipStream_t stream;
    int flags = 0;                  // XSQ_WIENER_SOFTMASK | XSQ_WIENER_RESIDUAL: J = 5 sources with the latter
    const float* sources = nullptr; // the oracle: the coefficients of the four true sources (arena of 8B channels) in place of X and
                                    // the starts; may be Y itself.  One iteration, no options.
};

static inline int sources_of(int flags) { return (flags & XSQ_WIENER_RESIDUAL) ? 5 : 4; }
static inline int slot_of(int J) { return J == 5 ? Slot<5>::N : Slot<4>::N; }
static inline int res_window_of(int J) { return J == 5 ? res_max_window<5> : res_max_window<4>; }

// f(integral_constant<int, J>, integral_constant<Start, ST>) for the call's option set; ST is the mixture phase where the
// estimates are given (the start is theirs)
template <bool MASKED, class Fn>
static void with_options(int flags, Fn&& f) {
    using Mix = std::integral_constant<Start, Start::MixPhase>;
    using Soft = std::integral_constant<Start, Start::Softmask>;
    using J4 = std::integral_constant<int, 4>;
    using J5 = std::integral_constant<int, 5>;
    if constexpr (MASKED) {
        if (flags & XSQ_WIENER_SOFTMASK) {
            if (sources_of(flags) == 5) f(J5{}, Soft{}); else f(J4{}, Soft{});
            return;
        }
    }
    if (sources_of(flags) == 5) f(J5{}, Mix{}); else f(J4{}, Mix{});
}

// the longest window a call runs: win_len, or the longest row when that is shorter
static int64_t longest_window(int nblocks, const int32_t* T, int S, int win_len) {
    int64_t maxN = 0;
    for (int k = 0; k < nblocks; ++k) maxN = std::max<int64_t>(maxN, (int64_t)S * T[k]);
    return std::min<int64_t>(win_len, maxN);
}

// statistics of J sources: one slot per (row, window)
static size_t stats_bytes(int nblocks, const int32_t* F, const int32_t* T, int Bn, int S, int win_len, int J) {
    if (nblocks <= 0 || !F || !T || Bn <= 0 || S <= 0 || win_len <= 0) return 0;
    int64_t stat = 0;
    for (int k = 0; k < nblocks; ++k)
        stat += (int64_t)Bn * F[k] * (((int64_t)S * T[k] + win_len - 1) / win_len) * slot_of(J);
    return (size_t)stat * 4 + 256;
}

// workspace of the iteration entry points: the statistics | max |x|^2 per (block, group, window) of the resident form
static size_t iter_stats_bytes(const EmCall& c) { return al256(stats_bytes(c.nblocks, c.F, c.T, c.Bn, c.S, c.win_len, sources_of(c.flags))); }
static size_t iter_bytes(int nblocks, const int32_t* F, const int32_t* T, int Bn, int S, int win_len, int J) {
    return al256(stats_bytes(nblocks, F, T, Bn, S, win_len, J)) + (size_t)xsq_wiener_num_windows(nblocks, F, T, Bn, S, win_len, 1) * 4 + 256;
}

// The argument checks of every forward entry point; no HIP call.  `masked`: the entry point takes masks; `iter`: it takes
// niter / method and the larger workspace.  Defaults batch_group; *resident: the form the call takes (niter >= 2).
static int check_em(const char* who, EmCall& c, bool masked, bool iter, int niter, int method, bool* resident) {
    if (int rc = check_table(who, c.nblocks, c.F, c.T, c.Bn, c.S)) return rc;
    XSQ_REQUIRE((c.X || c.sources) && c.Y && c.ws && (c.masks || !masked), "%s: null argument", who);
    // from sources: xsq_wiener_em_sources is the only caller and has no iteration count, flags or shared maximum to pass
    if (c.sources) XSQ_REQUIRE(((uintptr_t)c.sources | (uintptr_t)c.Y) % 16 == 0, "%s: the arenas must be 16-byte aligned", who);
    XSQ_REQUIRE((c.flags & ~(XSQ_WIENER_SOFTMASK | XSQ_WIENER_RESIDUAL)) == 0, "%s: flags=%d (XSQ_WIENER_SOFTMASK | XSQ_WIENER_RESIDUAL)", who, c.flags);
    const int J = sources_of(c.flags);
    if (masked) XSQ_REQUIRE(c.win_len > 0 && c.win_len % 2 == 0, "%s: win_len=%d must be even (two frames per thread)", who, c.win_len);
    XSQ_REQUIRE(c.win_len > 0, "%s: win_len=%d", who, c.win_len);
    XSQ_REQUIRE(niter != 0 || !masked || c.flags, "%s: niter=0 is the mix-phase estimate mask * X, which has no EM pass "
                                                  "(xsq_slicqt_inverse_masked forms it)", who);
    XSQ_REQUIRE(niter >= 0, "%s: niter=%d", who, niter);
    XSQ_REQUIRE(method >= 0 && method <= 2, "%s: method=%d (0 auto, 1 looped, 2 resident)", who, method);
    const int64_t longest = longest_window(c.nblocks, c.T, c.S, c.win_len);
    const bool fits = longest <= res_window_of(J);
    XSQ_REQUIRE(method != 2 || fits, "%s: the resident form holds windows of at most %d frames (this call's longest has %lld)", who,
                res_window_of(J), (long long)longest);
    if (c.batch_group <= 0) c.batch_group = c.Bn;
    XSQ_REQUIRE(c.Bn % c.batch_group == 0, "%s: batch_group=%d does not divide B=%d", who, c.batch_group, c.Bn);
    const size_t need = iter ? iter_bytes(c.nblocks, c.F, c.T, c.Bn, c.S, c.win_len, J) : stats_bytes(c.nblocks, c.F, c.T, c.Bn, c.S, c.win_len, J);
    XSQ_REQUIRE(c.ws_bytes >= need, "%s: workspace too small", who);
    for (int b = 0; masked && b < c.nblocks; ++b)
        XSQ_REQUIRE(((int64_t)c.S * c.T[b]) % 2 == 0, "%s: block %d has an odd frame count S*T=%lld", who, b, (long long)c.S * c.T[b]);
    *resident = niter >= 2 && method != 1 && fits;
    return XSQ_OK;
}

static void launch_window_max(const WTable& t, const float* X, float* ext_max, int Bn, int S, int win_len, hipStream_t stream) {
    XSQ_PROF("wiener_window_max", stream);
    hipLaunchKernelGGL(k_wiener_window_max, dim3(t.nwork), dim3(256), 0, stream, (const float2*)X, t.d_rows, t.d_work, t.d_bw_of_work,
                       ext_max, Bn, S, win_len);
}

// in place on Y; with masks (iteration 1 of the masked form) Y is only written
static void launch_apply(const WTable& t, const EmCall& c, const float* masks) {
    XSQ_PROF("wiener_apply", c.stream);
    if (c.sources)
        hipLaunchKernelGGL(k_wiener_apply_sources<true>, dim3((unsigned)(((t.max_frames + 1) / 2 + 255) / 256), t.nrows), dim3(256), 0, c.stream,
                           (const float2*)c.sources, (float2*)c.Y, t.d_rows, (const float*)c.ws, c.Bn, c.S, c.win_len);
    else if (masks)
        with_options<true>(c.flags, [&](auto j, auto st) {
            hipLaunchKernelGGL((k_wiener_apply_masked<decltype(j)::value, decltype(st)::value>), dim3((unsigned)((t.max_frames / 2 + 255) / 256), t.nrows),
                               dim3(256), 0, c.stream, (const float2*)c.X, masks, (float2*)c.Y, t.d_rows, (const float*)c.ws, c.Bn, c.S, c.win_len);
        });
    else
        with_options<false>(c.flags, [&](auto j, auto) {
            hipLaunchKernelGGL((k_wiener_apply<decltype(j)::value>), dim3((unsigned)((t.max_frames + 255) / 256), t.nrows), dim3(256), 0, c.stream,
                               (const float2*)c.X, (float2*)c.Y, t.d_rows, (const float*)c.ws, c.Bn, c.S, c.win_len);
        });
}

template <YFrom SRC>
static void launch_stats(const WTable& t, const EmCall& c) {
    XSQ_PROF(SRC == YFrom::Current ? "wiener_stats_iter" : "wiener_stats", c.stream);
    if constexpr (SRC == YFrom::Sources) {
        hipLaunchKernelGGL((k_wiener_stats<SRC, 4, Start::MixPhase>), dim3(t.nwork), dim3(256), 0, c.stream, nullptr, (const float2*)c.sources,
                           nullptr, t.d_rows, t.d_work, (float*)c.ws, c.Bn, c.S, c.win_len);
    } else {
        with_options<SRC == YFrom::Masks>(c.flags, [&](auto j, auto st) {
            hipLaunchKernelGGL((k_wiener_stats<SRC, decltype(j)::value, decltype(st)::value>), dim3(t.nwork), dim3(256), 0, c.stream,
                               (const float2*)c.X, (const float2*)c.Y, c.masks, t.d_rows, t.d_work, (float*)c.ws, c.Bn, c.S, c.win_len);
        });
    }
}

// the J starts of an option set into Y (2JB channels), from the masks or from magnitudes (a: real arena of 8B channels)
static int launch_start(const WTable& t, const float* X, const float* a, bool from_masks, float* Y, int Bn, int S, int flags, hipStream_t stream) {
    XSQ_PROF("wiener_start", stream);
    const dim3 grid((unsigned)((t.max_frames + 255) / 256), t.nrows);
    using Mix = std::integral_constant<Start, Start::MixPhase>;
    using Soft = std::integral_constant<Start, Start::Softmask>;
    auto go = [&](auto j, auto st) {
        constexpr int J = decltype(j)::value;
        constexpr Start ST = decltype(st)::value;
        if (from_masks) hipLaunchKernelGGL((k_wiener_start<J, ST, true>), grid, dim3(256), 0, stream, (const float2*)X, a, (float2*)Y, t.d_rows, Bn, S);
        else hipLaunchKernelGGL((k_wiener_start<J, ST, false>), grid, dim3(256), 0, stream, (const float2*)X, a, (float2*)Y, t.d_rows, Bn, S);
    };
    const bool soft = flags & XSQ_WIENER_SOFTMASK;
    if (sources_of(flags) == 5) { if (soft) go(std::integral_constant<int, 5>{}, Soft{}); else go(std::integral_constant<int, 5>{}, Mix{}); }
    else if (soft) go(std::integral_constant<int, 4>{}, Soft{});
    else { set_error("xsq_wiener_start: no option set (xsq_phasemix / mask * X is that start)"); return XSQ_ERR_ARG; }
    XSQ_HIP(hipGetLastError());
    return XSQ_OK;
}

// niter >= 1 iterations of the looped form: the three launches of iteration 1, then statistics + apply per further one (the
// estimates are in Y and 1/ma^2 in the stats slots by then)
static int run_em(const EmCall& c, int niter) {
    WTable t;
    const int J = sources_of(c.flags);
    if (int rc = get_wtable(c.nblocks, c.F, c.T, c.Bn, c.S, c.win_len, c.batch_group, &t, slot_of(J))) return rc;
    if (c.sources) launch_stats<YFrom::Sources>(t, c);
    else if (c.masks) launch_stats<YFrom::Masks>(t, c);
    else launch_stats<YFrom::Estimates>(t, c);
    { XSQ_PROF("wiener_finalize", c.stream);
    hipLaunchKernelGGL((J == 5 ? k_wiener_finalize<5> : k_wiener_finalize<4>), dim3(t.nblockwin), dim3(256), 0, c.stream, t.d_rows, t.d_blockwin,
                       (float*)c.ws, c.ext_max); }
    launch_apply(t, c, c.masks);
    for (int it = 2; it <= niter; ++it) {
        launch_stats<YFrom::Current>(t, c);
        launch_apply(t, c, nullptr);
    }
    XSQ_HIP(hipGetLastError());
    return XSQ_OK;
}

static int run_resident(const EmCall& c, int niter) {
    WTable t;
    if (int rc = get_wtable(c.nblocks, c.F, c.T, c.Bn, c.S, c.win_len, c.batch_group, &t, slot_of(sources_of(c.flags)))) return rc;
    float* wmax = (float*)((char*)c.ws + iter_stats_bytes(c));
    XSQ_HIP(hipMemsetAsync(wmax, 0, (size_t)t.nblockwin * 4, c.stream));
    launch_window_max(t, c.X, wmax, c.Bn, c.S, c.win_len, c.stream);
    { XSQ_PROF("wiener_resident", c.stream);
    auto go = [&](auto masked, auto j, auto st) {
        hipLaunchKernelGGL((k_wiener_resident<decltype(masked)::value, decltype(j)::value, decltype(st)::value>), dim3(t.nwork), dim3(RES_THREADS), 0,
                           c.stream, (const float2*)c.X, c.masks, (float2*)c.Y, t.d_rows, t.d_work, t.d_bw_of_work, wmax, c.ext_max, c.Bn, c.S,
                           c.win_len, niter);
    };
    if (c.masks) with_options<true>(c.flags, [&](auto j, auto st) { go(std::true_type{}, j, st); });
    else with_options<false>(c.flags, [&](auto j, auto st) { go(std::false_type{}, j, st); }); }
    XSQ_HIP(hipGetLastError());
    return XSQ_OK;
}

static int em(const char* who, EmCall c, bool masked, bool iter, int niter, int method) {
    bool resident;
    if (int rc = check_em(who, c, masked, iter, niter, method, &resident)) return rc;
    if (niter == 0) {                                     // the initial estimate is the result (norbert :247-251)
        if (!masked || !c.flags) return XSQ_OK;
        WTable t;
        if (int rc = get_wtable(c.nblocks, c.F, c.T, c.Bn, c.S, c.win_len, c.batch_group, &t, slot_of(sources_of(c.flags)))) return rc;
        return launch_start(t, c.X, c.masks, true, c.Y, c.Bn, c.S, c.flags, c.stream);
    }
    return resident ? run_resident(c, niter) : run_em(c, niter);
}

}  // namespace xsq

using namespace xsq;

extern "C" {

int xsq_phasemix(int nblocks, const int32_t* F, const int32_t* T, const float* X, const float* mag, float* Y,
                 int Bn, int S, void* stream_) {
    int rc = check_table("xsq_phasemix", nblocks, F, T, Bn, S);
    if (rc) return rc;
    XSQ_REQUIRE(X && mag && Y, "xsq_phasemix: null argument");
    WTable t;
    if ((rc = get_wtable(nblocks, F, T, Bn, S, 5000, Bn, &t))) return rc;
    hipLaunchKernelGGL(k_phasemix, dim3((unsigned)((t.max_frames + 255) / 256), t.nrows), dim3(256), 0,
                       (hipStream_t)stream_, (const float2*)X, mag, (float2*)Y, t.d_rows, Bn, S);
    XSQ_HIP(hipGetLastError());
    return XSQ_OK;
}

size_t xsq_wiener_workspace(int nblocks, const int32_t* F, const int32_t* T, int Bn, int S, int win_len) {
    return stats_bytes(nblocks, F, T, Bn, S, win_len, 4);
}

int64_t xsq_wiener_num_windows(int nblocks, const int32_t* F, const int32_t* T, int Bn, int S, int win_len, int batch_group) {
    if (nblocks <= 0 || !F || !T || Bn <= 0 || S <= 0 || win_len <= 0) return 0;
    if (batch_group <= 0) batch_group = Bn;
    if (Bn % batch_group) return 0;
    int64_t n = 0;
    for (int k = 0; k < nblocks; ++k) n += (int64_t)(Bn / batch_group) * (((int64_t)S * T[k] + win_len - 1) / win_len);
    return n;
}

int xsq_wiener_resident_max_window(void) { return res_max_window<4>; }

int xsq_wiener_resident_max_window_sources(int nsources) { return nsources == 4 || nsources == 5 ? res_window_of(nsources) : 0; }

size_t xsq_wiener_iter_workspace(int nblocks, const int32_t* F, const int32_t* T, int Bn, int S, int win_len, int niter, int method) {
    if (nblocks <= 0 || !F || !T || Bn <= 0 || S <= 0 || win_len <= 0 || niter < 0 || method < 0 || method > 2) return 0;
    return iter_bytes(nblocks, F, T, Bn, S, win_len, 4);
}

// ---- the option set: softmask start, residual fifth source (norbert.wiener use_softmask, norbert.contrib.residual_model) -----
size_t xsq_wiener_options_workspace(int nblocks, const int32_t* F, const int32_t* T, int Bn, int S, int win_len, int niter, int method,
                                    int flags) {
    if (nblocks <= 0 || !F || !T || Bn <= 0 || S <= 0 || win_len <= 0 || niter < 0 || method < 0 || method > 2 ||
        (flags & ~(XSQ_WIENER_SOFTMASK | XSQ_WIENER_RESIDUAL)))
        return 0;
    return iter_bytes(nblocks, F, T, Bn, S, win_len, sources_of(flags));
}

int xsq_wiener_start(int nblocks, const int32_t* F, const int32_t* T, const float* X, const float* mag, float* Y, int Bn, int S, int flags,
                     void* stream_) {
    int rc = check_table("xsq_wiener_start", nblocks, F, T, Bn, S);
    if (rc) return rc;
    XSQ_REQUIRE(X && mag && Y, "xsq_wiener_start: null argument");
    XSQ_REQUIRE(flags && (flags & ~(XSQ_WIENER_SOFTMASK | XSQ_WIENER_RESIDUAL)) == 0,
                "xsq_wiener_start: flags=%d (XSQ_WIENER_SOFTMASK | XSQ_WIENER_RESIDUAL, at least one)", flags);
    WTable t;
    if ((rc = get_wtable(nblocks, F, T, Bn, S, 5000, Bn, &t))) return rc;
    return launch_start(t, X, mag, false, Y, Bn, S, flags, (hipStream_t)stream_);
}

int xsq_wiener_em_options(int nblocks, const int32_t* F, const int32_t* T, const float* X, float* Y, int Bn, int S, int win_len,
                          int batch_group, int niter, int method, int flags, void* ws, size_t ws_bytes, void* stream_) {
    EmCall c{nblocks, F, T, X, nullptr, Y, Bn, S, win_len, batch_group, nullptr, ws, ws_bytes, (hipStream_t)stream_};
    c.flags = flags;
    return em("xsq_wiener_em_options", c, false, true, niter, method);
}

int xsq_wiener_em_masked_options(int nblocks, const int32_t* F, const int32_t* T, const float* X, const float* masks, float* Y, int Bn,
                                 int S, int win_len, int batch_group, const float* ext_max, int niter, int method, int flags, void* ws,
                                 size_t ws_bytes, void* stream_) {
    EmCall c{nblocks, F, T, X, masks, Y, Bn, S, win_len, batch_group, ext_max, ws, ws_bytes, (hipStream_t)stream_};
    c.flags = flags;
    return em("xsq_wiener_em_masked_options", c, true, true, niter, method);
}

int xsq_wiener_window_max(int nblocks, const int32_t* F, const int32_t* T, const float* X, int Bn, int S, int win_len,
                          int batch_group, float* ext_max, void* stream_) {
    int rc = check_table("xsq_wiener_window_max", nblocks, F, T, Bn, S);
    if (rc) return rc;
    XSQ_REQUIRE(X && ext_max && win_len > 0, "xsq_wiener_window_max: bad argument");
    if (batch_group <= 0) batch_group = Bn;
    XSQ_REQUIRE(Bn % batch_group == 0, "xsq_wiener_window_max: batch_group=%d does not divide B=%d", batch_group, Bn);
    WTable t;
    if ((rc = get_wtable(nblocks, F, T, Bn, S, win_len, batch_group, &t))) return rc;
    launch_window_max(t, X, ext_max, Bn, S, win_len, (hipStream_t)stream_);
    XSQ_HIP(hipGetLastError());
    return XSQ_OK;
}

// One iteration is the looped form at niter = 1 (method 1); the iteration entry points pass theirs on.
int xsq_wiener_em(int nblocks, const int32_t* F, const int32_t* T, const float* X, float* Y, int Bn, int S,
                  int win_len, int batch_group, void* ws, size_t ws_bytes, void* stream_) {
    return em("xsq_wiener_em", {nblocks, F, T, X, nullptr, Y, Bn, S, win_len, batch_group, nullptr, ws, ws_bytes, (hipStream_t)stream_},
              false, false, 1, 1);
}

int xsq_wiener_em_masked(int nblocks, const int32_t* F, const int32_t* T, const float* X, const float* masks, float* Y,
                         int Bn, int S, int win_len, int batch_group, void* ws, size_t ws_bytes, void* stream_) {
    return xsq_wiener_em_masked_ext(nblocks, F, T, X, masks, Y, Bn, S, win_len, batch_group, nullptr, ws, ws_bytes, stream_);
}

int xsq_wiener_em_masked_ext(int nblocks, const int32_t* F, const int32_t* T, const float* X, const float* masks, float* Y,
                             int Bn, int S, int win_len, int batch_group, const float* ext_max, void* ws, size_t ws_bytes,
                             void* stream_) {
    return em("xsq_wiener_em_masked", {nblocks, F, T, X, masks, Y, Bn, S, win_len, batch_group, ext_max, ws, ws_bytes, (hipStream_t)stream_},
              true, false, 1, 1);
}

// ---- the oracle's filter: fed by the coefficients of the four true sources (slicqfinder.py:43-117) -----------------------
// win_len == 0: one window over all the frames of a row, as the reference's blockwise_wiener takes it
static int whole_row_window(int nblocks, const int32_t* T, int S, int win_len) {
    if (win_len != 0 || nblocks <= 0 || !T || S <= 0) return win_len;
    return (int)std::min<int64_t>(std::max<int64_t>(longest_window(nblocks, T, S, INT32_MAX), 1), INT32_MAX);
}

size_t xsq_wiener_sources_workspace(int nblocks, const int32_t* F, const int32_t* T, int Bn, int S, int win_len) {
    return stats_bytes(nblocks, F, T, Bn, S, whole_row_window(nblocks, T, S, win_len), 4);
}

int xsq_wiener_em_sources(int nblocks, const int32_t* F, const int32_t* T, const float* Sc, float* Y, int Bn, int S, int win_len,
                          int batch_group, void* ws, size_t ws_bytes, void* stream_) {
    XSQ_REQUIRE(Sc, "xsq_wiener_em_sources: null argument");
    EmCall c{nblocks, F, T, nullptr, nullptr, Y, Bn, S, whole_row_window(nblocks, T, S, win_len), batch_group, nullptr, ws, ws_bytes,
             (hipStream_t)stream_};
    c.sources = Sc;
    return em("xsq_wiener_em_sources", c, false, false, 1, 1);
}

int xsq_phasemix_sources(int nblocks, const int32_t* F, const int32_t* T, const float* Sc, float* Y, int Bn, int S, void* stream_) {
    int rc = check_table("xsq_phasemix_sources", nblocks, F, T, Bn, S);
    if (rc) return rc;
    XSQ_REQUIRE(Sc && Y, "xsq_phasemix_sources: null argument");
    XSQ_REQUIRE(((uintptr_t)Sc | (uintptr_t)Y) % 16 == 0, "xsq_phasemix_sources: the arenas must be 16-byte aligned");
    WTable t;
    if ((rc = get_wtable(nblocks, F, T, Bn, S, 5000, Bn, &t))) return rc;
    XSQ_PROF("phasemix_sources", (hipStream_t)stream_);
    hipLaunchKernelGGL(k_wiener_apply_sources<false>, dim3((unsigned)(((t.max_frames + 1) / 2 + 255) / 256), t.nrows), dim3(256), 0,
                       (hipStream_t)stream_, (const float2*)Sc, (float2*)Y, t.d_rows, nullptr, Bn, S, 0);
    XSQ_HIP(hipGetLastError());
    return XSQ_OK;
}

// ---- niter iterations (norbert/__init__.py:133-148, 247-260) -----------------------------------------------------------
int xsq_wiener_em_iter(int nblocks, const int32_t* F, const int32_t* T, const float* X, float* Y, int Bn, int S, int win_len,
                       int batch_group, int niter, int method, void* ws, size_t ws_bytes, void* stream_) {
    return em("xsq_wiener_em_iter", {nblocks, F, T, X, nullptr, Y, Bn, S, win_len, batch_group, nullptr, ws, ws_bytes, (hipStream_t)stream_},
              false, true, niter, method);
}

int xsq_wiener_em_masked_iter(int nblocks, const int32_t* F, const int32_t* T, const float* X, const float* masks, float* Y, int Bn,
                              int S, int win_len, int batch_group, const float* ext_max, int niter, int method, void* ws,
                              size_t ws_bytes, void* stream_) {
    return em("xsq_wiener_em_masked_iter", {nblocks, F, T, X, masks, Y, Bn, S, win_len, batch_group, ext_max, ws, ws_bytes, (hipStream_t)stream_},
              true, true, niter, method);
}

}  // extern "C"
