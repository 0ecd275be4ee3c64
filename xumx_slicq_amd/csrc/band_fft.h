// The FFT band engine: analysis and synthesis of one band of length Lg = 4 m above LONG_LG, on plans created with
// XSQ_PLAN_LONG_BANDS (xsq_plan_create_flags).  Work O(Lg log Lg), tables linear in Lg; m is arbitrary (a prime, 113; a
// cube, 343; 4 * 401).
//
//   Y[k] = sum_q X[q] e^{sigma 2 pi i q k / Lg},  sigma = +1 analysis, -1 synthesis
// is split once by four (q = 4 q1 + r, k = k1 + m k2):
//   Y[k1 + m k2] = sum_r (sigma i)^{r k2} w^{r k1} A_r[k1],   A_r[k1] = sum_q1 X[4 q1 + r] e^{sigma 2 pi i q1 k1 / m},  w = e^{sigma 2 pi i / Lg}
// and each A_r is a chirp-z (Bluestein) transform of length m:  q1 k1 = (q1^2 + k1^2 - (k1 - q1)^2) / 2, so with the chirp
// c[j] = e^{sigma pi i j^2 / m}
//   A_r[k1] = c[k1] sum_q1 (X[4 q1 + r] c[q1]) conj(c)[k1 - q1]
// -- a linear convolution with conj(c) on -(m - 1) .. m - 1, run as a cyclic one of N >= 2 m - 1 points, N a power of two, inside
// LDS: a decimation-in-frequency FFT (natural order in, bit-reversed out), the product with the transformed chirp (built on the
// host in double, stored in bit-reversed order with the 1 / N), and a decimation-in-time inverse FFT (bit-reversed in, natural
// out): no reordering pass.  Pairs of radix-2 stages are fused into one pass over LDS.
//
// Tables, per band and direction, from PlanArgs::analysis_window / synthesis_window like every other engine's:
//   pre[q]   (Lg complex)  c[q / 4], times the analysis window of q in the analysis (the band's input is windowed)
//   post[r m + k1] (Lg complex)  c[k1] w^{r k1}, one rounding of the product formed in double
//   win[q]   (Lg real)     the synthesis window of q (the band's output is windowed); unused by the analysis
// and per distinct m / N: the transformed chirp (N complex), the twiddles e^{-2 pi i k / N}, k < N / 2.  j^2 is reduced mod 2 m,
// and r k1 mod Lg, in integers.
//
// One workgroup per (row, band); a launch per class of N, so that a band of N = 512 does not reserve the 64 KB of one of
// N = 8192.  The four A_r are parked on the band's own output row -- entry r m + k1 is written, and read back for the final
// radix-4 step, by the one lane that owns k1, and that step writes the four entries k1 + m k2 it has just read -- so the engine
// needs no workspace.  Fixed order throughout: the same bits every run.
#pragma once
#include "common.h"
#include "gemm_tile_bf3.h"

namespace xsq {

constexpr int LF_NT = 256;
constexpr int LF_MAX_N = 8192;                  // 64 KB of LDS: the largest static + dynamic allocation that needs no opt-in
constexpr int LF_MAX_LG = 4 * (LF_MAX_N / 2);   // N >= 2 m - 1 with m = Lg / 4: 16384 (xsq_plan_long_band_max)

struct LongBandDev {
    int Lg, m, N;          // N: power of two >= 2 m - 1, 8 <= N <= LF_MAX_N
    int bin0, f, F;        // as BandDev
    int jband;             // band index inside the plan (= row of the model's input_mean / input_scale tables), as Band4Dev's
    int64_t cum;
    int64_t pre_off, post_off, win_off, chirp_off, tw_off;     // float offsets into the direction's pool
};

struct LongArgs {
    const LongBandDev* bands;
    const float* pool;
    const float* in;       // analysis: slice spectra U (rows of nbins complex); synthesis: the coefficient (or mix) arena
    float* out;            // analysis: the coefficient arena; synthesis: Z (arena layout).  CONTRACT: `out` never overlaps `in` (nor `mask`):
                           // the kernel parks its four sub-transforms on the band's output row while it still reads the input
                           // row (forward_impl: U -> coef; inverse_impl: coef -> Z in the workspace).  `xin` lies in the CDAE's
                           // workspace and overlaps neither: it is only written, once per entry, after the last read of the parked row
    int BC, S, nbins, L;
    const float* mask;     // synthesis, optional: coefficients = mask * mix, `in` the mix arena of BCx channels
    int BCx;
    // analysis, optional: the CDAE's whitened magnitude (|coef| + mean[band]) * scale[band] written beside the coefficients, same
    // arena layout, real; split = 1: in the split-bf16 operand format -- Band4Args' fields of the same names (band_dft4.h)
    float* xin;
    const float* mean;
    const float* scale;
    int split;
};

__device__ __forceinline__ float2 lf_mul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ float2 lf_mulc(float2 a, float2 b) { return make_float2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y); }   // a conj(b)
__device__ __forceinline__ float2 lf_add(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 lf_sub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }

// forward FFT of buf[0 .. N), e^{-}: natural order in, bit-reversed order out.  tw[k] = e^{-2 pi i k / N}.  Ends on a barrier.
__device__ __forceinline__ void lf_fft_dif(float2* buf, int N, const float2* __restrict__ tw) {
    int s = N;
    for (; s >= 4; s >>= 2) {                    // the stages of block size s and s / 2
        const int qh = s >> 2, step = N / s;
        for (int p = threadIdx.x; p < (N >> 2); p += LF_NT) {
            const int blk = p / qh, j = p - blk * qh, i0 = blk * s + j;
            const float2 w1 = tw[j * step], w2 = tw[2 * j * step];
            const float2 x0 = buf[i0], x1 = buf[i0 + qh], x2 = buf[i0 + 2 * qh], x3 = buf[i0 + 3 * qh];
            const float2 y0 = lf_add(x0, x2), y1 = lf_add(x1, x3);
            const float2 y2 = lf_mul(lf_sub(x0, x2), w1);
            const float2 d = lf_sub(x1, x3);
            const float2 y3 = lf_mul(make_float2(d.y, -d.x), w1);          // (x1 - x3) (-i) w1: the twiddle of j + s / 4
            buf[i0] = lf_add(y0, y1);
            buf[i0 + qh] = lf_mul(lf_sub(y0, y1), w2);
            buf[i0 + 2 * qh] = lf_add(y2, y3);
            buf[i0 + 3 * qh] = lf_mul(lf_sub(y2, y3), w2);
        }
        __syncthreads();
    }
    if (s == 2) {                                // log2 N odd: the last stage, twiddle 1
        for (int p = threadIdx.x; p < (N >> 1); p += LF_NT) {
            const float2 u = buf[2 * p], v = buf[2 * p + 1];
            buf[2 * p] = lf_add(u, v);
            buf[2 * p + 1] = lf_sub(u, v);
        }
        __syncthreads();
    }
}

// inverse FFT, e^{+}, unnormalised: bit-reversed order in, natural order out -- lf_fft_dif's stages undone in reverse order.
__device__ __forceinline__ void lf_fft_dit_inv(float2* buf, int N, const float2* __restrict__ tw) {
    int s = 4;
    if (__builtin_ctz(N) & 1) {
        for (int p = threadIdx.x; p < (N >> 1); p += LF_NT) {
            const float2 u = buf[2 * p], v = buf[2 * p + 1];
            buf[2 * p] = lf_add(u, v);
            buf[2 * p + 1] = lf_sub(u, v);
        }
        __syncthreads();
        s = 8;
    }
    for (; s <= N; s <<= 2) {                    // the stages of block size s / 2 and s
        const int qh = s >> 2, step = N / s;
        for (int p = threadIdx.x; p < (N >> 2); p += LF_NT) {
            const int blk = p / qh, j = p - blk * qh, i0 = blk * s + j;
            const float2 w1 = tw[j * step], w2 = tw[2 * j * step];
            const float2 x0 = buf[i0], x1 = lf_mulc(buf[i0 + qh], w2), x2 = buf[i0 + 2 * qh], x3 = lf_mulc(buf[i0 + 3 * qh], w2);
            const float2 y0 = lf_add(x0, x1), y1 = lf_sub(x0, x1);
            const float2 y2 = lf_mulc(lf_add(x2, x3), w1);
            const float2 e = lf_mulc(lf_sub(x2, x3), w1);
            const float2 y3 = make_float2(-e.y, e.x);                      // (x2 - x3) conj(w1) (+i)
            buf[i0] = lf_add(y0, y2);
            buf[i0 + 2 * qh] = lf_sub(y0, y2);
            buf[i0 + qh] = lf_add(y1, y3);
            buf[i0 + 3 * qh] = lf_sub(y1, y3);
        }
        __syncthreads();
    }
}

// grid (rows, bands of the class), LF_NT threads, 8 N bytes of dynamic LDS.  `first`: the class's first entry of a.bands.
template <bool FWD>
__global__ __launch_bounds__(LF_NT) void k_band_fft(const LongArgs a, int first) {
    extern __shared__ __attribute__((aligned(16))) float2 lf_buf[];
    const LongBandDev b = a.bands[first + blockIdx.y];
    const int row = blockIdx.x, bc = row / a.S, s = row - bc * a.S;
    const int n = b.Lg, m = b.m, N = b.N;
    const float2* __restrict__ pre = reinterpret_cast<const float2*>(a.pool + b.pre_off);
    const float2* __restrict__ post = reinterpret_cast<const float2*>(a.pool + b.post_off);
    const float* __restrict__ win = a.pool + b.win_off;
    const float2* __restrict__ chirp = reinterpret_cast<const float2*>(a.pool + b.chirp_off);
    const float2* __restrict__ tw = reinterpret_cast<const float2*>(a.pool + b.tw_off);
    // complex entry of (bc, s) of this band in an arena of C channels
    const auto arena_row = [&](int C, int ch) { return (int64_t)C * a.S * b.cum + (((int64_t)ch * b.F + b.f) * a.S + s) * n; };
    float2* const orow = reinterpret_cast<float2*>(a.out) + arena_row(a.BC, bc);
    const float2* irow;
    const float* mrow = nullptr;
    if (FWD) irow = reinterpret_cast<const float2*>(a.in) + (int64_t)row * a.nbins;
    else if (a.mask) { irow = reinterpret_cast<const float2*>(a.in) + arena_row(a.BCx, bc % a.BCx); mrow = a.mask + arena_row(a.BC, bc); }
    else irow = reinterpret_cast<const float2*>(a.in) + arena_row(a.BC, bc);

    for (int r = 0; r < 4; ++r) {
        for (int i = threadIdx.x; i < N; i += LF_NT) {
            float2 v = make_float2(0.f, 0.f);
            if (i < m) {
                const int q = 4 * i + r;
                float2 x;
                if (FWD) {      // window index q -> spectrum position p -> bin, mirrored (and conjugated) outside [0, L/2]
                    int p = q + n / 2; p = p >= n ? p - n : p;
                    const int bin = b.bin0 + p;
                    const bool mir = bin < 0 || bin > a.L / 2;
                    x = irow[bin < 0 ? -bin : (bin > a.L / 2 ? a.L - bin : bin)];
                    if (mir) x.y = -x.y;
                } else {
                    x = irow[q];
                    if (mrow) { const float mk = mrow[q]; x.x *= mk; x.y *= mk; }
                }
                v = lf_mul(x, pre[q]);
            }
            lf_buf[i] = v;
        }
        __syncthreads();
        lf_fft_dif(lf_buf, N, tw);
        for (int i = threadIdx.x; i < N; i += LF_NT) lf_buf[i] = lf_mul(lf_buf[i], chirp[i]);
        __syncthreads();
        lf_fft_dit_inv(lf_buf, N, tw);
        for (int k1 = threadIdx.x; k1 < m; k1 += LF_NT) orow[r * m + k1] = lf_mul(lf_buf[k1], post[r * m + k1]);
        __syncthreads();
    }
    float* xrow = nullptr;                       // analysis: the band's row of the whitened magnitude (uniform)
    float w_mu = 0.f, w_sc = 1.f;
    if (FWD && a.xin) { xrow = a.xin + arena_row(a.BC, bc); w_mu = a.mean[b.jband]; w_sc = a.scale[b.jband]; }
    // the radix-4 step over what this lane parked: Y[k1 + m k2] = sum_r (sigma i)^{r k2} A_r[k1]
    for (int k1 = threadIdx.x; k1 < m; k1 += LF_NT) {
        const float2 a0 = orow[k1], a1 = orow[m + k1], a2 = orow[2 * m + k1], a3 = orow[3 * m + k1];
        const float2 s02 = lf_add(a0, a2), d02 = lf_sub(a0, a2), s13 = lf_add(a1, a3), d13 = lf_sub(a1, a3);
        const float2 id13 = FWD ? make_float2(-d13.y, d13.x) : make_float2(d13.y, -d13.x);      // (sigma i) (a1 - a3)
        float2 y[4] = {lf_add(s02, s13), lf_add(d02, id13), lf_sub(s02, s13), lf_sub(d02, id13)};
        if (FWD) {
#pragma unroll
            for (int k2 = 0; k2 < 4; ++k2) orow[k1 + m * k2] = y[k2];
            if (xrow) {         // the epilogue of band_dft4.h (FWD && a.xin): a split word depends on its own value alone
#pragma unroll
                for (int k2 = 0; k2 < 4; ++k2) {
                    const float wm = whiten_mag(y[k2].x, y[k2].y, w_mu, w_sc);
                    xrow[k1 + m * k2] = a.split ? bf3_word(wm) : wm;
                }
            }
        } else {        // window index q = k1 + m k2 lands on spectrum position (q + Lg / 2) mod Lg = k1 + m ((k2 + 2) mod 4)
#pragma unroll
            for (int k2 = 0; k2 < 4; ++k2) {
                const float g = win[k1 + m * k2];
                orow[k1 + m * ((k2 + 2) & 3)] = make_float2(y[k2].x * g, y[k2].y * g);
            }
        }
    }
}

}  // namespace xsq
