// Polyphase sinc resampling of fp32 rows, gfx950: the front end's rate conversion (data.py preprocess_audio ->
// torchaudio.transforms.Resample(rate, model_rate, "sinc_interpolation"), Hann window, 6 zero crossings, rolloff 0.99).
//
// torchaudio runs it as conv1d(x_pad, K, stride=o) with K of shape (n phases, 2*width + o taps) over the row padded with
// `width` zeros in front and `width + o` behind: y[j*n + p] = sum_k K[p][k] * x_pad[j*o + k].  Outside a window of about
// 12*o/base taps every entry of K is exactly 0 in fp32, so the host (xumx_slicq_amd/resample.py) keeps each phase's
// non-zero run only: table[p][0..span), whose first tap sits at k = first_tap[p].  Skipping an exact zero leaves an
// fp32 sum unchanged for finite input, so the result is the conv's with at most `span` FMAs per output.
//
// One workgroup owns RUN = 256 * R consecutive outputs of one row (R <= 8 is picked by the host so that the input the
// run needs fits the LDS segment), and the grid strides over (row, run) pairs.  Per run: the exact input range of the
// run's outputs (a workgroup min / max), a coalesced float4 staging of that range into LDS -- reads outside [0, len_in)
// are the padding's zeros, x_pad is never formed -- then `span` FMAs per output in ascending tap order against the
// table (in LDS when it fits, staged once per workgroup) and one coalesced dword store per output.  A run whose range
// would not fit the segment (only extreme downsampling ratios) reads its inputs from global memory instead.
#include "../../include/xumx_slicq_hip.h"
#include "common.h"
#include "prof.h"

#include <limits.h>
#include <algorithm>

namespace xsq {

constexpr int RS_THREADS = 256;
constexpr int RS_MAX_R = 8;                       // outputs per thread and run
constexpr int RS_SEG_CAP = 8192;                  // floats of the input segment (32 KiB)
constexpr int RS_TAB_CAP = 8192;                  // floats of the LDS table image incl. first_tap (32 KiB)
constexpr int RS_MAX_GRID = 2048;                 // 256 CUs x 8 workgroups

struct ResampleArgs {
    const float* x;
    const float* table;
    const int32_t* first_tap;
    float* y;
    int64_t x_stride, y_stride;
    int len_in, len_out;
    int o, n, span, width;
    int tstride;                                  // row stride of the LDS table image (odd: conflict-free column reads)
    int R;                                        // outputs per thread and run
    int runs;                                     // runs per row
    int total;                                    // rows * runs
    int seg_cap;                                  // floats of the LDS segment
};

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v = min(v, __shfl_xor(v, s));
    return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v = max(v, __shfl_xor(v, s));
    return v;
}

template <bool TLDS>
__global__ __launch_bounds__(RS_THREADS) void k_resample(ResampleArgs a) {
    extern __shared__ float4 smem4[];
    float* smem = reinterpret_cast<float*>(smem4);
    __shared__ int red[2][RS_THREADS / 64];
    const int t = threadIdx.x, wave = t >> 6;
    const int n = a.n, o = a.o, span = a.span;
    // LDS: [table image n x tstride][first_tap n] (TLDS only, rounded up to 4 floats) [segment]
    const int tab_floats = TLDS ? (n * a.tstride + n + 3) & ~3 : 0;
    float* tab_s = smem;
    int* first_s = reinterpret_cast<int*>(smem + (int64_t)n * a.tstride);
    float* seg = smem + tab_floats;
    if (TLDS) {
        for (int e = t; e < n * span; e += RS_THREADS) {
            const int p = e / span;
            tab_s[p * a.tstride + (e - p * span)] = a.table[e];
        }
        for (int p = t; p < n; p += RS_THREADS) first_s[p] = a.first_tap[p];
        __syncthreads();
    }
    const int RUN = RS_THREADS * a.R;
    const int dq = RS_THREADS / n, dr = RS_THREADS - dq * n;      // +256 outputs = +dq frames, +dr phases
    for (int w = blockIdx.x; w < a.total; w += gridDim.x) {
        const int row = w / a.runs, m0 = (w - row * a.runs) * RUN;
        const int mend = min(m0 + RUN, a.len_out);
        const float* xr = a.x + row * a.x_stride;
        float* yr = a.y + row * a.y_stride;
        // input start of each output this thread owns: x index j*o + first_tap[p] - width
        int j0 = (m0 + t) / n, p0 = (m0 + t) - j0 * n;
        int lo = INT_MAX, hi = INT_MIN;
        {
            int j = j0, p = p0;
            for (int r = 0, m = m0 + t; r < a.R && m < mend; ++r, m += RS_THREADS) {
                const int s = j * o + (TLDS ? first_s[p] : a.first_tap[p]) - a.width;
                lo = min(lo, s);
                hi = max(hi, s);
                p += dr; j += dq;
                if (p >= n) { p -= n; ++j; }
            }
        }
        lo = wave_min(lo);
        hi = wave_max(hi);
        if ((t & 63) == 0) { red[0][wave] = lo; red[1][wave] = hi; }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < RS_THREADS / 64; ++i) { lo = min(lo, red[0][i]); hi = max(hi, red[1][i]); }
        const int lo4 = lo & ~3;                                    // floor to a float4 boundary (also below 0)
        const int nseg = hi + span - lo4;                           // floats read: [lo4, hi + span)
        const bool staged = nseg <= a.seg_cap;
        if (staged) {
            const int nv = (nseg + 3) >> 2;
            const bool al = ((reinterpret_cast<uintptr_t>(xr) & 15) == 0);
            for (int v = t; v < nv; v += RS_THREADS) {
                const int g = lo4 + 4 * v;
                float4 q;
                if (al && g >= 0 && g + 4 <= a.len_in) {
                    q = *reinterpret_cast<const float4*>(xr + g);
                } else {                                             // the row's ends: zero padding, unaligned rows
                    q.x = (g >= 0 && g < a.len_in) ? xr[g] : 0.f;
                    q.y = (g + 1 >= 0 && g + 1 < a.len_in) ? xr[g + 1] : 0.f;
                    q.z = (g + 2 >= 0 && g + 2 < a.len_in) ? xr[g + 2] : 0.f;
                    q.w = (g + 3 >= 0 && g + 3 < a.len_in) ? xr[g + 3] : 0.f;
                }
                reinterpret_cast<float4*>(seg)[v] = q;
            }
        }
        __syncthreads();
        {
            int j = j0, p = p0;
            for (int r = 0, m = m0 + t; r < a.R && m < mend; ++r, m += RS_THREADS) {
                const int s = j * o + (TLDS ? first_s[p] : a.first_tap[p]) - a.width;
                const float* tp = TLDS ? tab_s + p * a.tstride : a.table + (int64_t)p * span;
                float acc = 0.f;
                if (staged) {
                    const float* xs = seg + (s - lo4);
#pragma unroll 4
                    for (int i = 0; i < span; ++i) acc = fmaf(tp[i], xs[i], acc);
                } else {
                    for (int i = 0; i < span; ++i) {
                        const int g = s + i;
                        acc = fmaf(tp[i], (g >= 0 && g < a.len_in) ? xr[g] : 0.f, acc);
                    }
                }
                yr[m] = acc;
                p += dr; j += dq;
                if (p >= n) { p -= n; ++j; }
            }
        }
        __syncthreads();                                            // the segment and red[] are reused by the next run
    }
}

}  // namespace xsq

using namespace xsq;

extern "C" int xsq_resample(const float* x, int64_t x_stride, int rows, int64_t len_in, float* y, int64_t y_stride,
                            int64_t len_out, const float* table, const int32_t* first_tap, int o, int n, int span,
                            int width, void* stream) {
    XSQ_REQUIRE(x && y && table && first_tap, "xsq_resample: null pointer");
    XSQ_REQUIRE(rows >= 0 && len_in >= 0 && len_out >= 0, "xsq_resample: rows %d, len_in %lld, len_out %lld", rows,
                (long long)len_in, (long long)len_out);
    XSQ_REQUIRE(o >= 1 && n >= 1 && span >= 1 && width >= 0, "xsq_resample: o %d, n %d, span %d, width %d", o, n, span,
                width);
    XSQ_REQUIRE((int64_t)n * span < (1ll << 31), "xsq_resample: table of %d x %d entries", n, span);
    // every output reads inputs j*o + first_tap[p] - width + [0, span) with j <= len_out / n and first_tap < 2*width + o:
    // all of it, and every output index, must fit 32-bit signed arithmetic
    const int64_t frames = len_out / n + 1;
    XSQ_REQUIRE(len_out + RS_THREADS * RS_MAX_R < (1ll << 31) && len_in < (1ll << 31) &&
                    frames * o + 2ll * width + o + span + 4 < (1ll << 31),
                "xsq_resample: len_in %lld / len_out %lld exceed 32-bit offsets", (long long)len_in, (long long)len_out);
    XSQ_REQUIRE(rows <= 1 || (x_stride >= len_in && y_stride >= len_out), "xsq_resample: row strides %lld / %lld",
                (long long)x_stride, (long long)y_stride);
    if (rows == 0 || len_out == 0) return XSQ_OK;
    // outputs per thread and run: the most (<= 8) whose input range fits the segment.  That range is at most
    // (RUN - 1) * o / n + 2 * width + span + 4 floats (each phase's non-zero taps lie within 6 * o / base <= width of its
    // centre); a run that still exceeds it takes the kernel's global-memory path.
    int R = RS_MAX_R;
    auto seg_need = [&](int r) { return ((int64_t)RS_THREADS * r - 1) * o / n + 2ll * width + span + 8; };
    while (R > 1 && seg_need(R) > RS_SEG_CAP) --R;
    const int seg_cap = (int)((std::min<int64_t>(seg_need(R), RS_SEG_CAP) + 3) & ~3ll);
    const int tstride = span | 1;
    const int64_t tab_floats = round_up((int64_t)n * tstride + n, 4);
    const bool tlds = tab_floats <= RS_TAB_CAP;
    const int64_t runs = (len_out + (int64_t)RS_THREADS * R - 1) / ((int64_t)RS_THREADS * R);
    XSQ_REQUIRE(runs * rows < (1ll << 31), "xsq_resample: %d rows x %lld runs", rows, (long long)runs);
    ResampleArgs a{x, table, first_tap, y, x_stride, y_stride, (int)len_in, (int)len_out, o, n, span, width, tstride, R,
                   (int)runs, (int)(runs * rows), seg_cap};
    const size_t lds = sizeof(float) * (size_t)(seg_cap + (tlds ? tab_floats : 0));
    const unsigned grid = (unsigned)std::min<int64_t>(runs * rows, RS_MAX_GRID);
    hipStream_t st = (hipStream_t)stream;
    XSQ_PROF("resample", st);
    if (tlds)
        hipLaunchKernelGGL(k_resample<true>, dim3(grid), dim3(RS_THREADS), lds, st, a);
    else
        hipLaunchKernelGGL(k_resample<false>, dim3(grid), dim3(RS_THREADS), lds, st, a);
    XSQ_HIP(hipGetLastError());
    return XSQ_OK;
}
