// The mirrored synthesis of the bands that reach across DC, and its transpose (plans made by xsq_plan_create_twins).
//
// The reference's inverse synthesises every inner band a second time through the dual window of its negative-frequency mirror
// (nsgt/nsigtf.py:57-99, quirk A12 of DESIGN.md section 2).  For a band j with 0 < c_j < Lg_j / 2 that lands on kept bins:
//   fr_s[q - c_j] += (-1)^(c_j/2) (-1)^q (-i on even slices s, +i on odd) Lg_j gd'_j[q] conj( FFT_Lg(coef_{s,j})[q + 1] ),
//   c_j <= q < Lg_j / 2,  gd'_j[q] = gd_j[Lg_j - q]
// (the q + 1 is the reference's off-by-one; s counts inside the transform of its own channel).  At bins 0 and L/2 only the real
// part is added: irfft ignores the imaginary one.  A handful of entries per slice (Bark-28 and Bark-56: 6 + 2 on bins 0..5), so
// both kernels are one small workgroup per row (bc, s): one lane owns a bin (synthesis) or a coefficient (analysis) and sums its
// entries in table order -- no atomics, the same bits every run.
#pragma once
#include "common.h"

namespace xsq {

struct TwinDst { int at, first, count, tw; };   // synthesis: at = landing bin; analysis: at = band (tw: its twiddles).  Entries [first, first + count)
struct TwinSrc { int at, q1, tw; float w; };    // synthesis: at = band; analysis: at = bin.  q1 = q + 1; w: the real weight, 1/L (and the irfft weight) folded in

// complex offset of row (bc, s) of band b in an arena of C channels
__device__ __forceinline__ int64_t twin_row(const BandDev& b, int C, int S, int bc, int s) {
    return (int64_t)C * S * b.cum + (((int64_t)bc * b.F + b.f) * S + s) * b.Lg;
}

// grid (BC * S), 64 threads.  fr: the slice spectra k_spectrum_gather left, in front of the inverse FFT.  Coefficients as
// BandInvOp reads them: the arena, or mask[bc] * mix[bc % BCx] (the product rounded to fp32 first, as there).
__global__ __launch_bounds__(64) void k_twin_synthesis(const float* __restrict__ coef, const float* __restrict__ mask, int BCx,
                                                       const BandDev* __restrict__ bands, const TwinDst* __restrict__ dst,
                                                       const TwinSrc* __restrict__ src, const float2* __restrict__ tw, int ndst,
                                                       float2* __restrict__ fr, int BC, int S, int nbins) {
    const int row = blockIdx.x;
    const int bc = row / S, s = row - bc * S;
    const float rot = (s & 1) ? 1.f : -1.f;                 // +i on odd slices, -i on even ones
    for (int i = threadIdx.x; i < ndst; i += 64) {
        const TwinDst d = dst[i];
        float2* const out = fr + (int64_t)row * nbins + d.at;
        float2 acc = *out;
        for (int e = d.first; e < d.first + d.count; ++e) {
            const TwinSrc t = src[e];
            const BandDev b = bands[t.at];
            const float* p = coef + 2 * (mask ? twin_row(b, BCx, S, bc % BCx, s) : twin_row(b, BC, S, bc, s));
            const float* mk = mask ? mask + twin_row(b, BC, S, bc, s) : nullptr;
            float dr = 0.f, di = 0.f;                       // FFT_Lg(coef)[q + 1]
            int r = 0;                                      // (q + 1) t mod Lg
            for (int t0 = 0; t0 < b.Lg; t0 += 2) {          // two coefficients per 16-byte load (Lg % 4 == 0)
                float4 v = *reinterpret_cast<const float4*>(p + 2 * t0);
                if (mk) {
                    const float2 m = *reinterpret_cast<const float2*>(mk + t0);
                    v.x *= m.x; v.y *= m.x; v.z *= m.y; v.w *= m.y;
                }
                const float2 w0 = tw[t.tw + r];
                r += t.q1; r -= r >= b.Lg ? b.Lg : 0;
                const float2 w1 = tw[t.tw + r];
                r += t.q1; r -= r >= b.Lg ? b.Lg : 0;
                dr += v.x * w0.x + v.y * w0.y; di += v.y * w0.x - v.x * w0.y;     // times e^{-i theta}
                dr += v.z * w1.x + v.w * w1.y; di += v.w * w1.x - v.z * w1.y;
            }
            // w (-+i) conj(D) = -+w (Di + i Dr)
            acc.x += rot * t.w * di;
            if (d.at != 0 && d.at != nbins - 1) acc.y += rot * t.w * dr;
        }
        *out = acc;
    }
}

// The transpose, for xsq_slicqt_inverse_adjoint: grid (BC * S), 64 threads.  V: the slice spectra of gy (rfft_L, slice window of
// ones) the analysis kernels ran on; gcoef: the gradient arena they wrote, BC channels.  The entry weights carry the irfft
// weights (1 at bins 0 and L/2, else 2) over L.  With A = (-+i) conj(V[k]):  gcoef[t] += w A e^{+2 pi i (q + 1) t / Lg}.
__global__ __launch_bounds__(64) void k_twin_analysis(const float2* __restrict__ V, const BandDev* __restrict__ bands,
                                                      const TwinDst* __restrict__ dst, const TwinSrc* __restrict__ src,
                                                      const float2* __restrict__ tw, int ndst, float* __restrict__ gcoef, int BC, int S,
                                                      int nbins) {
    const int row = blockIdx.x;
    const int bc = row / S, s = row - bc * S;
    const float rot = (s & 1) ? 1.f : -1.f;
    for (int i = 0; i < ndst; ++i) {
        const TwinDst d = dst[i];
        const BandDev b = bands[d.at];
        float2* const g = reinterpret_cast<float2*>(gcoef) + twin_row(b, BC, S, bc, s);
        for (int t0 = threadIdx.x; t0 < b.Lg; t0 += 64) {
            float2 acc = g[t0];
            for (int e = d.first; e < d.first + d.count; ++e) {
                const TwinSrc t = src[e];
                const float2 v = V[(int64_t)row * nbins + t.at];
                const float ar = rot * v.y, ai = rot * v.x;                      // (-+i) conj(V) = -+(Vi + i Vr)
                const float2 w = tw[d.tw + (int)(((int64_t)t.q1 * t0) % b.Lg)];
                acc.x += t.w * (ar * w.x - ai * w.y);
                acc.y += t.w * (ar * w.y + ai * w.x);
            }
            g[t0] = acc;
        }
    }
}

}  // namespace xsq
